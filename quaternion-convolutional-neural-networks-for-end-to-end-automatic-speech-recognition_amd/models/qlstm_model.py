"""TIMIT model with quaternion LSTM layers (Parcollet et al., "Quaternion Recurrent Neural Networks", ICLR 2019): the same
filter-bank input, output layer and CTC pipeline as TimitQCNN, with a stack of (bidirectional) QuaternionLSTM layers in place
of the convolutions and TimeDistributed dense layers.  The reference has no such model; no phone error rate has been measured
with it."""
import torch

from ..complexnn import QuaternionLayerNormalization, QuaternionLSTM
from ..keras_like import regularizers
from ..layers import Dense, Dropout, TimeDistributed, ctc_batch_cost, dense_softmax_ctc_mean
from .interspeech_model import TimitQCNN


class TimitQLSTM(TimitQCNN):
    """x (B, 4, F, T) -- the quaternion filter-bank input of TimitQCNN (F = 41: 40 filters + energy; r = 0, i / j / k = static,
    delta, delta-delta) -- is viewed as (B, T, 4 * F): component-major r|i|j|k, as every quaternion layer here reads its input.
    `num_layers` QuaternionLSTM(units) layers follow, Dropout between them, then TimeDistributed(Dense(62, softmax)).
    layer_norm=True puts one QuaternionLayerNormalization behind every recurrent layer (`self.norm`), in front of the next layer's
    dropout and with the same `lengths`; without it no such module, parameter or state_dict key exists.

    The decoding / scoring surface (ctc_loss, ctc_mean_loss, decode, evaluate, error_breakdown, align, transcribe,
    regularization_loss, training_loss) is TimitQCNN's; `input_length` is also handed to the recurrent layers as `lengths`, so
    that padding frames neither move the state nor, in the backward direction, come before an utterance's last frame."""

    def __init__(self, num_layers=4, units=1024, bidirectional=True, dropout=0.2, l2=0.0, layer_norm=False):
        torch.nn.Module.__init__(self)
        reg = regularizers.l2(l2) if l2 else None
        self.rate = dropout
        self.rnn = torch.nn.ModuleList([QuaternionLSTM(units, bidirectional=bidirectional, kernel_regularizer=reg,
                                                       recurrent_regularizer=reg, seed=1337 + 16 * i, name='qlstm%d' % i)
                                        for i in range(num_layers)])
        self.layer_norm = bool(layer_norm)
        if self.layer_norm:
            self.norm = torch.nn.ModuleList([QuaternionLayerNormalization(name='qlnorm%d' % i) for i in range(num_layers)])
        self.drop = Dropout(dropout)
        self.pred = TimeDistributed(Dense(62, activation='softmax', kernel_regularizer=reg, use_bias=True,
                                          bias_initializer='zeros', kernel_initializer='random_uniform'))
        self._lengths = None

    def features(self, x, input_length=None):
        """(B, 4, F, T) -> (B, T, D * units): the input of the output layer."""
        if x.dim() != 4 or x.shape[1] != 4:
            raise ValueError('TimitQLSTM expects (batch, 4, features, frames) input, got %s' % (tuple(x.shape),))
        lengths = input_length if input_length is not None else self._lengths
        if lengths is not None:
            lengths = lengths.reshape(-1).to(device=x.device, dtype=torch.int32)
        b, _, f, t = x.shape
        o = x.permute(0, 3, 1, 2).reshape(b, t, 4 * f)
        for i, layer in enumerate(self.rnn):
            if i:
                o = self.drop(o)
            o = layer(o, lengths=lengths)
            if self.layer_norm:
                o = self.norm[i](o, lengths=lengths)
        return o

    def forward(self, x, input_length=None):
        return self.pred(self.features(x, input_length))

    def _with_lengths(self, input_length, fn):
        """fn() with `input_length` as the recurrent layers' lengths for every forward pass inside it."""
        self._lengths = input_length
        try:
            return fn()
        finally:
            self._lengths = None

    def ctc_loss(self, x, labels, input_length, label_length, loss_scale=1.0):
        return ctc_batch_cost(self(x, input_length), labels, input_length, label_length, loss_scale=loss_scale)

    def ctc_mean_loss(self, x, labels, input_length, label_length, loss_scale=1.0):
        if not (x.is_cuda and x.dtype in (torch.bfloat16, torch.float16)):
            return self.ctc_loss(x, labels, input_length, label_length, loss_scale=loss_scale).mean()
        feats = self.features(x, input_length)
        dense = self.pred.layer
        dense.ensure_built((None, feats.shape[-1]), x.device)
        loss = dense_softmax_ctc_mean(feats, dense, labels, input_length, label_length, loss_scale)
        if loss is None:          # a width the fused output layer does not take
            loss = ctc_batch_cost(self.pred(feats), labels, input_length, label_length, loss_scale=loss_scale).mean()
        return loss

    def decode(self, x, input_length=None, **kw):
        return self._with_lengths(input_length, lambda: super(TimitQLSTM, self).decode(x, input_length, **kw))

    def align(self, x, labels, input_length=None, label_length=None):
        return self._with_lengths(input_length, lambda: super(TimitQLSTM, self).align(x, labels, input_length, label_length))

    def evaluate(self, x, labels, input_length, label_length, **kw):
        return self._with_lengths(input_length, lambda: super(TimitQLSTM, self).evaluate(x, labels, input_length, label_length, **kw))

    def error_breakdown(self, x, labels, input_length, label_length, **kw):
        return self._with_lengths(input_length,
                                  lambda: super(TimitQLSTM, self).error_breakdown(x, labels, input_length, label_length, **kw))
