"""Quaternion multi-head self-attention and a pre-norm transformer encoder block on the MI355X HIP path (include/qk_attn.h;
csrc/qk_qattn.hip).

The reference has no attention layer.  This one follows its conventions: `units` is the TOTAL real width (4 Q), tensors are laid out
r|i|j|k, both projections are the dense table conj(W) (x) x of QuaternionDense, every weight is drawn by qdense_init.

    qkv = quaternion_dense(x, kernel) + bias               ONE dense call: 3 Q quaternion units, q | k | v inside every component
    o   = qattention_packed(qkv, heads, lengths)           softmax_{t' < n}(<q_t, k_t'> / sqrt(4 dq)) v per head, read in place
    y   = quaternion_dense(o, out_kernel) + out_bias

The score <q_t, k_t'> is the real part of the quaternion inner product over a head's dq units; the weights are real, so every value
quaternion is scaled as a whole (the component-wise Hamilton scores of Tay et al., ACL 2019, are deliberately not built).
"""
import numpy as np
import torch

from .. import functional as F
from ..keras_like import InputSpec, Layer, regularizers
from .dense import QuaternionDense
from .init import qdense_init
from .norm import QuaternionLayerNormalization


class _QKVBlocks(object):
    """Initialiser of the (in_q, 4 * 3Q) projection: the q, k and v blocks, (in_q, 4 Q) each, are drawn independently by qdense_init
    and laid into the component-major layout (component p holds q | k | v at columns p * 3Q + [0, Q), [Q, 2Q), [2Q, 3Q))."""

    def __init__(self, in_q, q_units, criterion, seed):
        self.in_q, self.q_units, self.criterion, self.seed = in_q, q_units, criterion, seed

    def __call__(self, shape=None, dtype=None):
        q = self.q_units
        out = np.zeros((self.in_q, 12 * q))
        for g in range(3):
            block = qdense_init((self.in_q, q), self.criterion, seed=self.seed + g)()
            for p in range(4):
                out[:, p * 3 * q + g * q:p * 3 * q + (g + 1) * q] = block[:, p * q:(p + 1) * q]
        return out


class QuaternionMultiHeadAttention(Layer):
    """Input (B, T, 4 * in_q); output (B, T, units), units = 4 Q, Q = heads * dq.  `layer(x, lengths=)` with lengths (B,) int32: rows
    with t >= lengths[b] are never attended to and carry no attention output (y is out_bias there) and no gradient.
    Weights: kernel (in_q, 4 * 3Q), bias (4 * 3Q,), out_kernel (Q, 4 Q), out_bias (4 Q,).  dq of 16 or 32 runs on the matrix cores
    (bf16 / fp16)."""

    def __init__(self, units, heads, use_bias=True, init_criterion='he', kernel_regularizer=None, seed=None, name=None, **kwargs):
        if name is not None:
            kwargs['name'] = name
        super(QuaternionMultiHeadAttention, self).__init__(**kwargs)
        if units % 4 or units <= 0:
            raise ValueError('QuaternionMultiHeadAttention needs units divisible by 4, got %r' % (units,))
        if heads < 1 or (units // 4) % heads:
            raise ValueError('QuaternionMultiHeadAttention needs heads dividing the %d quaternion units, got %r' % (units // 4, heads))
        self.units, self.q_units, self.heads = units, units // 4, int(heads)
        self.use_bias, self.init_criterion = bool(use_bias), init_criterion
        self.kernel_regularizer = regularizers.get(kernel_regularizer)
        self.seed = int(np.random.randint(1, 10e6)) if seed is None else seed
        self.input_spec = InputSpec(ndim=3)

    def build(self, input_shape):
        assert len(input_shape) == 3
        width = input_shape[-1]
        if width is None or width % 4:
            raise ValueError('QuaternionMultiHeadAttention needs an input width divisible by 4, got %r' % (width,))
        in_q, Q = width // 4, self.q_units
        self.add_weight('kernel', (in_q, 12 * Q), initializer=_QKVBlocks(in_q, Q, self.init_criterion, self.seed),
                        regularizer=self.kernel_regularizer)
        if self.use_bias:
            self.add_weight('bias', (12 * Q,), initializer='zeros')
        else:
            self.bias = None
        self.add_weight('out_kernel', (Q, 4 * Q), initializer=qdense_init((Q, Q), self.init_criterion, seed=self.seed + 3),
                        regularizer=self.kernel_regularizer)
        if self.use_bias:
            self.add_weight('out_bias', (4 * Q,), initializer='zeros')
        else:
            self.out_bias = None
        self.input_spec = InputSpec(ndim=3, axes={-1: width})
        self.built = True

    def forward(self, inputs, lengths=None):
        self.ensure_built(inputs.shape, inputs.device)
        return self.call(inputs, lengths=lengths)

    def call(self, inputs, lengths=None):
        if inputs.dim() != 3:
            raise ValueError('%s expects (batch, time, features) input, got %s' % (self.name, tuple(inputs.shape)))
        b, t, width = inputs.shape
        qkv = F.quaternion_dense(inputs.reshape(b * t, width), self.kernel, self.bias).view(b, t, 3 * self.units)
        o = F.qattention_packed(qkv, self.heads, lengths=lengths)
        return F.quaternion_dense(o.view(b * t, self.units), self.out_kernel, self.out_bias).view(b, t, self.units)

    def compute_output_shape(self, input_shape):
        assert input_shape and len(input_shape) == 3
        return (input_shape[0], input_shape[1], self.units)

    def get_config(self):
        cfg = super(QuaternionMultiHeadAttention, self).get_config()
        cfg.update(units=self.units, heads=self.heads, use_bias=self.use_bias, init_criterion=self.init_criterion,
                   kernel_regularizer=regularizers.serialize(self.kernel_regularizer), seed=self.seed)
        return cfg


class QuaternionTransformerEncoderLayer(Layer):
    """Pre-norm encoder block on (B, T, units), all of it with the same `lengths`:

        x = x + Drop(MHA(QLN(x)))
        x = x + Drop(Dense(units)(relu(Dense(ff_units)(QLN(x)))))

    QLN is QuaternionLayerNormalization, MHA QuaternionMultiHeadAttention, Dense QuaternionDense.  Sub-layers: norm1, attention, norm2,
    ff1, ff2.  At rows t >= lengths[b] the normalisations give zeros and the attention reads nothing, so what such rows hold never
    reaches an active row."""

    def __init__(self, units, heads, ff_units, dropout=0.0, kernel_regularizer=None, seed=None, name=None, **kwargs):
        if name is not None:
            kwargs['name'] = name
        super(QuaternionTransformerEncoderLayer, self).__init__(**kwargs)
        if ff_units % 4 or ff_units <= 0:
            raise ValueError('QuaternionTransformerEncoderLayer needs ff_units divisible by 4, got %r' % (ff_units,))
        self.units, self.heads, self.ff_units, self.rate = units, int(heads), ff_units, float(dropout)
        self.kernel_regularizer = regularizers.get(kernel_regularizer)
        self.seed = int(np.random.randint(1, 10e6)) if seed is None else seed
        self.norm1 = QuaternionLayerNormalization(name=self.name + '_norm1')
        self.attention = QuaternionMultiHeadAttention(units, heads, kernel_regularizer=kernel_regularizer, seed=self.seed,
                                                      name=self.name + '_attention')
        self.norm2 = QuaternionLayerNormalization(name=self.name + '_norm2')
        self.ff1 = QuaternionDense(ff_units, activation='relu', kernel_regularizer=kernel_regularizer, seed=self.seed + 4,
                                   name=self.name + '_ff1')
        self.ff2 = QuaternionDense(units, kernel_regularizer=kernel_regularizer, seed=self.seed + 5, name=self.name + '_ff2')
        self.input_spec = InputSpec(ndim=3)

    def build(self, input_shape):
        assert len(input_shape) == 3
        if input_shape[-1] != self.units:
            raise ValueError('QuaternionTransformerEncoderLayer(units=%d) needs an input of that width, got %r' % (self.units, input_shape[-1]))
        for layer, shape in ((self.norm1, input_shape), (self.attention, input_shape), (self.norm2, input_shape),
                             (self.ff1, (None, self.units)), (self.ff2, (None, self.ff_units))):
            layer.ensure_built(shape, self._build_device)
        self.input_spec = InputSpec(ndim=3, axes={-1: self.units})
        self.built = True

    def forward(self, inputs, lengths=None):
        self.ensure_built(inputs.shape, inputs.device)
        return self.call(inputs, lengths=lengths)

    def call(self, inputs, lengths=None):
        b, t, width = inputs.shape
        x = inputs + torch.nn.functional.dropout(self.attention(self.norm1(inputs, lengths=lengths), lengths=lengths), self.rate, self.training)
        h = self.ff2(self.ff1(self.norm2(x, lengths=lengths).view(b * t, width))).view(b, t, width)
        return x + torch.nn.functional.dropout(h, self.rate, self.training)

    def compute_output_shape(self, input_shape):
        return tuple(input_shape)

    def get_config(self):
        cfg = super(QuaternionTransformerEncoderLayer, self).get_config()
        cfg.update(units=self.units, heads=self.heads, ff_units=self.ff_units, dropout=self.rate,
                   kernel_regularizer=regularizers.serialize(self.kernel_regularizer), seed=self.seed)
        return cfg
