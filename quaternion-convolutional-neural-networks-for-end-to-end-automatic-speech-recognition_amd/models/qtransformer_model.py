"""TIMIT model with quaternion self-attention: the same filter-bank input, output layer and CTC pipeline as TimitQCNN, with a
stack of pre-norm QuaternionTransformerEncoderLayer blocks in place of the convolutions.  The reference has no such model; no
phone error rate has been measured with it."""
import math

import torch

from ..complexnn import QuaternionDense, QuaternionLayerNormalization, QuaternionTransformerEncoderLayer
from ..keras_like import regularizers
from ..layers import Dense, Dropout, TimeDistributed
from .qlstm_model import TimitQLSTM


def sinusoidal_positions(steps, width):
    """(steps, width) float32: sin / cos of t / 10000^(2i / width) in even / odd columns -- fixed, not a parameter."""
    t = torch.arange(steps, dtype=torch.float32).unsqueeze(1)
    freq = torch.exp(torch.arange(0, width, 2, dtype=torch.float32) * (-math.log(10000.0) / width))
    table = torch.zeros(steps, width)
    table[:, 0::2] = torch.sin(t * freq)
    table[:, 1::2] = torch.cos(t * freq)[:, :width // 2]
    return table


class TimitQTransformer(TimitQLSTM):
    """x (B, 4, F, T) -- the quaternion filter-bank input of TimitQCNN -- is viewed as (B, T, 4 * F), projected by
    QuaternionDense(units) (`embed`), a fixed sinusoidal position table is added, `num_layers` pre-norm encoder blocks (`blocks`)
    follow, then a final QuaternionLayerNormalization (`final_norm`) and TimeDistributed(Dense(62, softmax)) (`pred`).
    units = 4 * heads * dq; dq of 16 or 32 (units = 64 * heads or 128 * heads) runs the attention on the matrix cores in bf16 / fp16.

    The loss / decoding / scoring surface is TimitQCNN's through TimitQLSTM: `input_length` is handed to every block as `lengths`,
    so padding frames are never attended to and the posteriors of a frame t < input_length[b] do not depend on what the padding
    frames hold."""

    def __init__(self, num_layers=6, units=512, heads=8, ff_units=2048, dropout=0.1, l2=0.0):
        torch.nn.Module.__init__(self)
        reg = regularizers.l2(l2) if l2 else None
        self.rate, self.units = dropout, units
        self.embed = QuaternionDense(units, kernel_regularizer=reg, seed=1301, name='qtf_embed')
        self.blocks = torch.nn.ModuleList([QuaternionTransformerEncoderLayer(units, heads, ff_units, dropout=dropout, kernel_regularizer=reg,
                                                                             seed=1337 + 16 * i, name='qtf%d' % i)
                                           for i in range(num_layers)])
        self.final_norm = QuaternionLayerNormalization(name='qtf_norm')
        self.drop = Dropout(dropout)
        self.pred = TimeDistributed(Dense(62, activation='softmax', kernel_regularizer=reg, use_bias=True,
                                          bias_initializer='zeros', kernel_initializer='random_uniform'))
        self._lengths = None
        self._positions = None

    def positions(self, steps, device, dtype):
        """The first `steps` rows of the position table on `device` in `dtype` (kept between calls; not in the state_dict)."""
        p = self._positions
        if p is None or p.shape[0] < steps or p.device != device or p.dtype != dtype:
            p = self._positions = sinusoidal_positions(steps, self.units).to(device=device, dtype=dtype)
        return p[:steps]

    def features(self, x, input_length=None):
        """(B, 4, F, T) -> (B, T, units): the input of the output layer."""
        if x.dim() != 4 or x.shape[1] != 4:
            raise ValueError('TimitQTransformer expects (batch, 4, features, frames) input, got %s' % (tuple(x.shape),))
        lengths = input_length if input_length is not None else self._lengths
        if lengths is not None:
            lengths = lengths.reshape(-1).to(device=x.device, dtype=torch.int32)
        b, _, f, t = x.shape
        o = self.embed(x.permute(0, 3, 1, 2).reshape(b * t, 4 * f)).view(b, t, self.units)
        o = self.drop(o + self.positions(t, o.device, o.dtype))
        for block in self.blocks:
            o = block(o, lengths=lengths)
        return self.final_norm(o, lengths=lengths)
