"""TIMIT model with quaternion Conformer blocks: the embedding projection, position table, output layer and CTC pipeline of
TimitQTransformer, with macaron QuaternionConformerBlock blocks -- self-attention plus a gated depthwise quaternion convolution
over time -- in place of the pre-norm transformer blocks.  The reference has no such model.  Nobody has measured a phone error
rate with it."""
import torch

from ..complexnn import QuaternionConformerBlock, QuaternionDense
from ..keras_like import regularizers
from ..layers import Dense, Dropout, TimeDistributed
from .qtransformer_model import TimitQTransformer


class TimitQConformer(TimitQTransformer):
    """x (B, 4, F, T) is viewed as (B, T, 4 * F), projected by QuaternionDense(units) (`embed`), the fixed sinusoidal position table
    is added, `num_layers` QuaternionConformerBlock blocks (`blocks`) follow -- each ends in its own QuaternionLayerNormalization, so
    there is no `final_norm` -- then TimeDistributed(Dense(62, softmax)) (`pred`).  units = 256 with 4 heads is dq = 16: the
    matrix-core attention path in bf16 / fp16.  `input_length` is handed to every block as `lengths`: padding frames are never
    attended to nor convolved over, and the posteriors of a frame t < input_length[b] do not depend on what the padding frames hold."""

    def __init__(self, num_layers=6, units=256, heads=4, ff_units=1024, kernel_size=15, dropout=0.1, l2=0.0):
        torch.nn.Module.__init__(self)
        reg = regularizers.l2(l2) if l2 else None
        self.rate, self.units = dropout, units
        self.embed = QuaternionDense(units, kernel_regularizer=reg, seed=1301, name='qcf_embed')
        self.blocks = torch.nn.ModuleList([QuaternionConformerBlock(units, heads, ff_units, kernel_size=kernel_size, dropout=dropout,
                                                                    kernel_regularizer=reg, seed=1337 + 32 * i, name='qcf%d' % i)
                                           for i in range(num_layers)])
        self.drop = Dropout(dropout)
        self.pred = TimeDistributed(Dense(62, activation='softmax', kernel_regularizer=reg, use_bias=True,
                                          bias_initializer='zeros', kernel_initializer='random_uniform'))
        self._lengths = None
        self._positions = None

    def features(self, x, input_length=None):
        """(B, 4, F, T) -> (B, T, units): the input of the output layer."""
        if x.dim() != 4 or x.shape[1] != 4:
            raise ValueError('TimitQConformer expects (batch, 4, features, frames) input, got %s' % (tuple(x.shape),))
        lengths = input_length if input_length is not None else self._lengths
        if lengths is not None:
            lengths = lengths.reshape(-1).to(device=x.device, dtype=torch.int32)
        b, _, f, t = x.shape
        o = self.embed(x.permute(0, 3, 1, 2).reshape(b * t, 4 * f)).view(b, t, self.units)
        o = self.drop(o + self.positions(t, o.device, o.dtype))
        for block in self.blocks:
            o = block(o, lengths=lengths)
        return o
