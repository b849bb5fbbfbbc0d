"""Quaternion layer normalisation on the MI355X HIP path (include/qk_norm.h; csrc/qk_qlnorm.hip).

The reference has no normalisation layer.  This one works per row of a component-major r|i|j|k tensor (..., 4 Q): the four component
means are removed, ONE variance over all 4 Q values scales the row, and ONE gamma per quaternion unit is shared by its four
components -- every quaternion is scaled as a whole and the ratios between its components survive.

    mu_c = mean_u x[c, u];  var = mean_{c, u} (x[c, u] - mu_c)^2;  y[c, u] = gamma[u] (x[c, u] - mu_c) / sqrt(var + epsilon) + beta[c, u]

It is the same in training and evaluation, keeps no running statistics and needs no collective.
"""
from .. import functional as F
from ..keras_like import InputSpec, Layer, initializers


class QuaternionLayerNormalization(Layer):
    """Input (..., 4 Q), output of the same shape.  Weights: gamma (Q,) when `scale`, beta (4 Q,) when `center`; neither carries a
    regulariser.  `layer(x, lengths=)` with x (B, T, 4 Q) and lengths (B,) int32: rows with t >= lengths[b] are inactive -- output
    exactly zero (not beta), no gradient -- the convention of QuaternionLSTM, so padding frames stay zero through a stack."""

    def __init__(self, epsilon=1e-3, center=True, scale=True, beta_initializer='zeros', gamma_initializer='ones', name=None, **kwargs):
        if name is not None:
            kwargs['name'] = name
        super(QuaternionLayerNormalization, self).__init__(**kwargs)
        if not epsilon >= 0:
            raise ValueError('QuaternionLayerNormalization needs epsilon >= 0, got %r' % (epsilon,))
        self.epsilon, self.center, self.scale = float(epsilon), bool(center), bool(scale)
        self.beta_initializer = initializers.get(beta_initializer)
        self.gamma_initializer = initializers.get(gamma_initializer)
        self.input_spec = InputSpec(min_ndim=1)

    def build(self, input_shape):
        width = input_shape[-1]
        if width is None or width % 4 or width <= 0:
            raise ValueError('QuaternionLayerNormalization needs a last axis divisible by 4, got %r' % (width,))
        if self.scale:
            self.add_weight('gamma', (width // 4,), initializer=self.gamma_initializer)
        if self.center:
            self.add_weight('beta', (width,), initializer=self.beta_initializer)
        self.input_spec = InputSpec(min_ndim=1, axes={-1: width})
        self.built = True

    def forward(self, inputs, lengths=None):
        self.ensure_built(inputs.shape, inputs.device)
        return self.call(inputs, lengths=lengths)

    def call(self, inputs, lengths=None):
        return F.qlayer_norm(inputs, self.gamma if self.scale else None, self.beta if self.center else None, lengths=lengths,
                             epsilon=self.epsilon)

    def compute_output_shape(self, input_shape):
        return tuple(input_shape)

    def get_config(self):
        cfg = super(QuaternionLayerNormalization, self).get_config()
        cfg.update(epsilon=self.epsilon, center=self.center, scale=self.scale,
                   beta_initializer=initializers.serialize(self.beta_initializer),
                   gamma_initializer=initializers.serialize(self.gamma_initializer))
        return cfg
