"""Depthwise quaternion convolution over time, the Conformer convolution module and the Conformer block on the MI355X HIP path
(include/qk_dwconv.h; csrc/qk_qdwconv.hip).

The reference has no such layers.  They follow its conventions: widths are TOTAL real widths (4 Q), tensors are laid out r|i|j|k,
the pointwise projections are QuaternionDense, the depthwise product is W (x) x as in its convolution layers, and every weight is
drawn by the polar quaternion initialiser of complexnn/init.py.

    u = pw1(x)                                          ONE dense call: 2 Q quaternion units, a | g inside every component
    h = qglu_dwconv1d(u, kernel, bias, lengths)         (a * sigmoid(g)) convolved over time, K quaternion taps per unit, one kernel
    y = pw2(silu(QLN(h)))
"""
import numpy as np
import torch

from .. import functional as F
from ..keras_like import InputSpec, Layer, regularizers
from .attention import QuaternionMultiHeadAttention
from .dense import QuaternionDense
from .init import qdense_init
from .norm import QuaternionLayerNormalization


class _GLUBlocks(object):
    """Initialiser of the (in_q, 4 * 2Q) gated projection: the a and g blocks, (in_q, 4 Q) each, are drawn independently by
    qdense_init and laid into the component-major layout (component p holds a | g at columns p * 2Q + [0, Q), [Q, 2Q))."""

    def __init__(self, in_q, q_units, criterion, seed):
        self.in_q, self.q_units, self.criterion, self.seed = in_q, q_units, criterion, seed

    def __call__(self, shape=None, dtype=None):
        q = self.q_units
        out = np.zeros((self.in_q, 8 * q))
        for g in range(2):
            block = qdense_init((self.in_q, q), self.criterion, seed=self.seed + g)()
            for p in range(4):
                out[:, p * 2 * q + g * q:p * 2 * q + (g + 1) * q] = block[:, p * q:(p + 1) * q]
        return out


class QuaternionDepthwiseConv1D(Layer):
    """Input (B, T, 4 Q) -- with `gated` the packed (B, T, 8 Q) output of a 2 Q-unit projection, a | g inside every component, which
    is gated a * sigmoid(g) inside the kernel -- and output (B, T, 4 Q).  Every quaternion unit has its own `kernel_size` quaternion
    taps: weights kernel (K, 4 Q), component-major per tap, and bias (4 Q,).  padding 'same' or 'causal'.  `layer(x, lengths=)` with
    lengths (B,) int32: the sequence is zero outside [0, lengths[b]) whatever x holds there, and rows t >= lengths[b] give zeros
    and take no gradient.  The kernel is drawn by qdense_init at the fan-in of a depthwise layer: K quaternion inputs per output
    (he: s = 1 / sqrt(2 K))."""

    def __init__(self, kernel_size, padding='same', gated=False, use_bias=True, init_criterion='he', kernel_regularizer=None, seed=None,
                 name=None, **kwargs):
        if name is not None:
            kwargs['name'] = name
        super(QuaternionDepthwiseConv1D, self).__init__(**kwargs)
        if not 1 <= int(kernel_size) <= 31:
            raise ValueError('QuaternionDepthwiseConv1D needs kernel_size in 1 .. 31, got %r' % (kernel_size,))
        F.qdwconv_pad_lo(kernel_size, padding)                  # raises for an unknown padding
        self.kernel_size, self.padding, self.gated = int(kernel_size), padding, bool(gated)
        self.use_bias, self.init_criterion = bool(use_bias), init_criterion
        self.kernel_regularizer = regularizers.get(kernel_regularizer)
        self.seed = int(np.random.randint(1, 10e6)) if seed is None else seed
        self.input_spec = InputSpec(ndim=3)

    def build(self, input_shape):
        assert len(input_shape) == 3
        width, mult = input_shape[-1], 8 if self.gated else 4
        if width is None or width <= 0 or width % mult:
            raise ValueError('QuaternionDepthwiseConv1D(gated=%s) needs a last axis divisible by %d, got %r' % (self.gated, mult, width))
        Q = width // mult
        self.add_weight('kernel', (self.kernel_size, 4 * Q), initializer=qdense_init((self.kernel_size, Q), self.init_criterion, seed=self.seed),
                        regularizer=self.kernel_regularizer)
        if self.use_bias:
            self.add_weight('bias', (4 * Q,), initializer='zeros')
        else:
            self.bias = None
        self.input_spec = InputSpec(ndim=3, axes={-1: width})
        self.built = True

    def forward(self, inputs, lengths=None):
        self.ensure_built(inputs.shape, inputs.device)
        return self.call(inputs, lengths=lengths)

    def call(self, inputs, lengths=None):
        fn = F.qglu_dwconv1d if self.gated else F.qdwconv1d
        return fn(inputs, self.kernel, self.bias, lengths=lengths, padding=self.padding)

    def compute_output_shape(self, input_shape):
        assert input_shape and len(input_shape) == 3
        return (input_shape[0], input_shape[1], input_shape[2] // 2 if self.gated else input_shape[2])

    def get_config(self):
        cfg = super(QuaternionDepthwiseConv1D, self).get_config()
        cfg.update(kernel_size=self.kernel_size, padding=self.padding, gated=self.gated, use_bias=self.use_bias,
                   init_criterion=self.init_criterion, kernel_regularizer=regularizers.serialize(self.kernel_regularizer), seed=self.seed)
        return cfg


class QuaternionConformerConvModule(Layer):
    """The convolution module of a Conformer block (Gulati et al., Interspeech 2020) on (B, T, units):

        y = pw2(swish(QLN(qglu_dwconv1d(pw1(x)))))

    pw1 is QuaternionDense(2 * units) whose kernel holds two independently drawn blocks a | g inside every component, pw2
    QuaternionDense(units), QLN QuaternionLayerNormalization, swish torch.nn.functional.silu.  Sub-layers: pw1, depthwise, norm, pw2.
    Deviation: Conformer's batch normalisation is replaced by QuaternionLayerNormalization -- the `layer_norm` option of ESPnet /
    NeMo -- which keeps the module independent of the batch and of padding.  With `lengths`, rows t >= lengths[b] are never read by
    the convolution and leave the normalisation as zeros (pw2 then gives its bias there, as every dense layer does)."""

    def __init__(self, units, kernel_size=15, padding='same', init_criterion='he', kernel_regularizer=None, seed=None, name=None, **kwargs):
        if name is not None:
            kwargs['name'] = name
        super(QuaternionConformerConvModule, self).__init__(**kwargs)
        if units % 4 or units <= 0:
            raise ValueError('QuaternionConformerConvModule needs units divisible by 4, got %r' % (units,))
        self.units, self.kernel_size, self.padding, self.init_criterion = units, int(kernel_size), padding, init_criterion
        self.kernel_regularizer = regularizers.get(kernel_regularizer)
        self.seed = int(np.random.randint(1, 10e6)) if seed is None else seed
        self.pw1 = QuaternionDense(2 * units, init_criterion=init_criterion, kernel_regularizer=kernel_regularizer, seed=self.seed,
                                   name=self.name + '_pw1')
        self.depthwise = QuaternionDepthwiseConv1D(kernel_size, padding=padding, gated=True, init_criterion=init_criterion,
                                                   kernel_regularizer=kernel_regularizer, seed=self.seed + 2, name=self.name + '_depthwise')
        self.norm = QuaternionLayerNormalization(name=self.name + '_norm')
        self.pw2 = QuaternionDense(units, init_criterion=init_criterion, kernel_regularizer=kernel_regularizer, seed=self.seed + 3,
                                   name=self.name + '_pw2')
        self.input_spec = InputSpec(ndim=3)

    def build(self, input_shape):
        assert len(input_shape) == 3
        if input_shape[-1] != self.units:
            raise ValueError('QuaternionConformerConvModule(units=%d) needs an input of that width, got %r' % (self.units, input_shape[-1]))
        fresh = not self.pw1.built
        for layer, shape in ((self.pw1, (None, self.units)), (self.depthwise, (None, None, 2 * self.units)),
                             (self.norm, (None, None, self.units)), (self.pw2, (None, self.units))):
            layer.ensure_built(shape, self._build_device)
        if fresh:                       # QuaternionDense always draws ONE qdense_init block: lay the two gate blocks over it
            blocks = _GLUBlocks(self.units // 4, self.units // 4, self.init_criterion, self.seed)()
            with torch.no_grad():
                self.pw1.r.copy_(torch.tensor(blocks, dtype=torch.float32))
        self.input_spec = InputSpec(ndim=3, axes={-1: self.units})
        self.built = True

    def forward(self, inputs, lengths=None):
        self.ensure_built(inputs.shape, inputs.device)
        return self.call(inputs, lengths=lengths)

    def call(self, inputs, lengths=None):
        b, t, width = inputs.shape
        u = self.pw1(inputs.reshape(b * t, width)).view(b, t, 2 * width)
        h = self.norm(self.depthwise(u, lengths=lengths), lengths=lengths)
        return self.pw2(torch.nn.functional.silu(h).view(b * t, width)).view(b, t, width)

    def compute_output_shape(self, input_shape):
        return tuple(input_shape)

    def get_config(self):
        cfg = super(QuaternionConformerConvModule, self).get_config()
        cfg.update(units=self.units, kernel_size=self.kernel_size, padding=self.padding, init_criterion=self.init_criterion,
                   kernel_regularizer=regularizers.serialize(self.kernel_regularizer), seed=self.seed)
        return cfg


class QuaternionConformerBlock(Layer):
    """The macaron Conformer block on (B, T, units), all of it with the same `lengths`:

        x = x + 1/2 Drop(FF1(QLN(x)))
        x = x + Drop(MHA(QLN(x)))
        x = x + Drop(Conv(QLN(x)))
        x = x + 1/2 Drop(FF2(QLN(x)))
        y = QLN(x)

    FF is Dense(units)(relu(Dense(ff_units)(.))) of QuaternionDense layers, MHA QuaternionMultiHeadAttention, Conv
    QuaternionConformerConvModule.  Sub-layers: norm_ff1, ff1_in, ff1_out, norm_mha, attention, norm_conv, conv, norm_ff2, ff2_in,
    ff2_out, norm_out.  Deviations from Gulati et al.: the feed-forward layers use relu where Conformer uses swish (relu stays fused
    in the dense kernel), and the convolution module normalises with QuaternionLayerNormalization instead of batch normalisation."""

    def __init__(self, units, heads, ff_units, kernel_size=15, dropout=0.0, padding='same', kernel_regularizer=None, seed=None, name=None,
                 **kwargs):
        if name is not None:
            kwargs['name'] = name
        super(QuaternionConformerBlock, self).__init__(**kwargs)
        if ff_units % 4 or ff_units <= 0:
            raise ValueError('QuaternionConformerBlock needs ff_units divisible by 4, got %r' % (ff_units,))
        self.units, self.heads, self.ff_units, self.kernel_size = units, int(heads), ff_units, int(kernel_size)
        self.rate, self.padding = float(dropout), padding
        self.kernel_regularizer = regularizers.get(kernel_regularizer)
        self.seed = int(np.random.randint(1, 10e6)) if seed is None else seed
        dense = lambda n, act, k, tag: QuaternionDense(n, activation=act, kernel_regularizer=kernel_regularizer, seed=self.seed + k,
                                                       name=self.name + tag)
        norm = lambda tag: QuaternionLayerNormalization(name=self.name + tag)
        self.norm_ff1, self.ff1_in, self.ff1_out = norm('_norm_ff1'), dense(ff_units, 'relu', 0, '_ff1_in'), dense(units, None, 1, '_ff1_out')
        self.norm_mha = norm('_norm_mha')
        self.attention = QuaternionMultiHeadAttention(units, heads, kernel_regularizer=kernel_regularizer, seed=self.seed + 2,
                                                      name=self.name + '_attention')
        self.norm_conv = norm('_norm_conv')
        self.conv = QuaternionConformerConvModule(units, kernel_size, padding=padding, kernel_regularizer=kernel_regularizer,
                                                  seed=self.seed + 6, name=self.name + '_conv')
        self.norm_ff2, self.ff2_in, self.ff2_out = norm('_norm_ff2'), dense(ff_units, 'relu', 10, '_ff2_in'), dense(units, None, 11, '_ff2_out')
        self.norm_out = norm('_norm_out')
        self.input_spec = InputSpec(ndim=3)

    def build(self, input_shape):
        assert len(input_shape) == 3
        if input_shape[-1] != self.units:
            raise ValueError('QuaternionConformerBlock(units=%d) needs an input of that width, got %r' % (self.units, input_shape[-1]))
        seq, row, wide = tuple(input_shape), (None, self.units), (None, self.ff_units)
        for layer, shape in ((self.norm_ff1, seq), (self.ff1_in, row), (self.ff1_out, wide), (self.norm_mha, seq), (self.attention, seq),
                             (self.norm_conv, seq), (self.conv, seq), (self.norm_ff2, seq), (self.ff2_in, row), (self.ff2_out, wide),
                             (self.norm_out, seq)):
            layer.ensure_built(shape, self._build_device)
        self.input_spec = InputSpec(ndim=3, axes={-1: self.units})
        self.built = True

    def forward(self, inputs, lengths=None):
        self.ensure_built(inputs.shape, inputs.device)
        return self.call(inputs, lengths=lengths)

    def call(self, inputs, lengths=None):
        b, t, width = inputs.shape
        drop = lambda v: torch.nn.functional.dropout(v, self.rate, self.training)
        ff = lambda norm, fin, fout, v: fout(fin(norm(v, lengths=lengths).view(b * t, width))).view(b, t, width)
        x = inputs + 0.5 * drop(ff(self.norm_ff1, self.ff1_in, self.ff1_out, inputs))
        x = x + drop(self.attention(self.norm_mha(x, lengths=lengths), lengths=lengths))
        x = x + drop(self.conv(self.norm_conv(x, lengths=lengths), lengths=lengths))
        x = x + 0.5 * drop(ff(self.norm_ff2, self.ff2_in, self.ff2_out, x))
        return self.norm_out(x, lengths=lengths)

    def compute_output_shape(self, input_shape):
        return tuple(input_shape)

    def get_config(self):
        cfg = super(QuaternionConformerBlock, self).get_config()
        cfg.update(units=self.units, heads=self.heads, ff_units=self.ff_units, kernel_size=self.kernel_size, dropout=self.rate,
                   padding=self.padding, kernel_regularizer=regularizers.serialize(self.kernel_regularizer), seed=self.seed)
        return cfg
