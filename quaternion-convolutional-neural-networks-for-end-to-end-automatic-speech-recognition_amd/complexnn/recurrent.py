"""Quaternion LSTM layer on the MI355X HIP path (Parcollet et al., "Quaternion Recurrent Neural Networks", ICLR 2019).

The reference has no recurrent layer; this one follows its conventions: `units` is the TOTAL real width, states and outputs are
laid out r|i|j|k, every product is the dense table conj(W) (x) x of QuaternionDense, every weight is drawn by qdense_init.

    zx  = quaternion_dense(x_t, kernel) + bias                         one dense call over all (B * T) rows (qk_dense_fwd)
    z_t = zx_t + quaternion_dense(h_{t-1}, recurrent_kernel)           the recurrence: functional.qlstm (include/qk_rnn.h)
    i, f, o = sigmoid(z_t[gate 0, 1, 3]);  g = tanh(z_t[gate 2]);  c_t = f c_{t-1} + i g;  h_t = o tanh(c_t)

Column layout of the 4 * units gate columns: component-major blocks of `units`, gate-major (i|f|g|o) inside a block.
"""
import numpy as np
import torch

from .. import functional as F
from ..keras_like import InputSpec, Layer, regularizers
from .init import qdense_init


class _GateBlocks(object):
    """Initialiser of a (in_q, 4 * units) weight [with a leading direction axis]: each gate's (in_q, 4 * q_units) block is drawn
    independently by qdense_init and laid into the component-major / gate-major column layout."""

    def __init__(self, in_q, q_units, directions, stacked, criterion, seed):
        self.in_q, self.q_units, self.directions, self.stacked, self.criterion, self.seed = in_q, q_units, directions, stacked, criterion, seed

    def __call__(self, shape=None, dtype=None):
        q, units = self.q_units, 4 * self.q_units
        out = np.zeros((self.directions, self.in_q, 4 * units))
        for d in range(self.directions):
            for g in range(4):
                block = qdense_init((self.in_q, q), self.criterion, seed=self.seed + 4 * d + g)()
                for p in range(4):
                    out[d, :, p * units + g * q:p * units + (g + 1) * q] = block[:, p * q:(p + 1) * q]
        return out if self.stacked else out[0]


class _GateBias(object):
    def __init__(self, q_units, directions, stacked, forget_one):
        self.q_units, self.directions, self.stacked, self.forget_one = q_units, directions, stacked, forget_one

    def __call__(self, shape=None, dtype=None):
        q, units = self.q_units, 4 * self.q_units
        out = np.zeros((self.directions, 4 * units))
        if self.forget_one:
            for c in range(4):
                out[:, c * units + q:c * units + 2 * q] = 1.0
        return out if self.stacked else out[0]


class QuaternionLSTM(Layer):
    """Input (B, T, 4 * in_q); output (B, T, D * units) (return_sequences) or (B, D * units), D = 2 when bidirectional.

    With two directions the output is the quaternion concatenation: component c, direction d, unit u at column
    c * (D * q_units) + d * q_units + u, written in place by the kernels.  go_backwards (one direction) walks t = T-1 .. 0; the
    output stays in time order (y[:, t] is the state after the steps t, t+1, ...).  `lengths` (B,) int32: rows are inactive from
    t = lengths[b] on -- state carried, output zero, no gradient; the backward direction starts at each row's own last frame.
    Weights: kernel (in_q, 4 * units), recurrent_kernel (q_units, 4 * units), bias (4 * units,), each with a leading direction
    axis when bidirectional.  The forget-gate bias starts at 1 in all four components (unit_forget_bias)."""

    def __init__(self, units, return_sequences=True, return_state=False, go_backwards=False, bidirectional=False,
                 unit_forget_bias=True, init_criterion='he', kernel_regularizer=None, recurrent_regularizer=None, seed=None, **kwargs):
        super(QuaternionLSTM, self).__init__(**kwargs)
        if units % 4 or units <= 0:
            raise ValueError('QuaternionLSTM needs units divisible by 4, got %r' % (units,))
        if go_backwards and bidirectional:
            raise ValueError('QuaternionLSTM: go_backwards applies to one direction; a bidirectional layer already has it')
        self.units, self.q_units = units, units // 4
        self.return_sequences, self.return_state = bool(return_sequences), bool(return_state)
        self.go_backwards, self.bidirectional = bool(go_backwards), bool(bidirectional)
        self.unit_forget_bias, self.init_criterion = bool(unit_forget_bias), init_criterion
        self.kernel_regularizer = regularizers.get(kernel_regularizer)
        self.recurrent_regularizer = regularizers.get(recurrent_regularizer)
        self.seed = int(np.random.randint(1, 10e6)) if seed is None else seed
        self.directions = 2 if self.bidirectional else 1
        self.input_spec = InputSpec(ndim=3)

    def build(self, input_shape):
        assert len(input_shape) == 3
        width = input_shape[-1]
        if width % 4:
            raise ValueError('QuaternionLSTM needs an input width divisible by 4, got %d' % width)
        in_q, D, st = width // 4, self.directions, self.bidirectional
        lead = (D,) if st else ()
        self.add_weight('kernel', lead + (in_q, 4 * self.units),
                        initializer=_GateBlocks(in_q, self.q_units, D, st, self.init_criterion, self.seed),
                        regularizer=self.kernel_regularizer)
        self.add_weight('recurrent_kernel', lead + (self.q_units, 4 * self.units),
                        initializer=_GateBlocks(self.q_units, self.q_units, D, st, self.init_criterion, self.seed + 8),
                        regularizer=self.recurrent_regularizer)
        self.add_weight('bias', lead + (4 * self.units,), initializer=_GateBias(self.q_units, D, st, self.unit_forget_bias))
        self.input_spec = InputSpec(ndim=3, axes={-1: width})
        self.built = True

    def forward(self, inputs, lengths=None, initial_state=None):
        self.ensure_built(inputs.shape, inputs.device)
        return self.call(inputs, lengths=lengths, initial_state=initial_state)

    def call(self, inputs, lengths=None, initial_state=None):
        if inputs.dim() != 3:
            raise ValueError('%s expects (batch, time, features) input, got %s' % (self.name, tuple(inputs.shape)))
        b, t, width = inputs.shape
        D, U = self.directions, self.units
        x2 = inputs.reshape(b * t, width)
        if self.bidirectional:
            zx = torch.stack([F.quaternion_dense(x2, self.kernel[d], self.bias[d]).view(b, t, 4 * U) for d in range(D)])
            R = self.recurrent_kernel
        else:
            zx = F.quaternion_dense(x2, self.kernel, self.bias).view(1, b, t, 4 * U)
            R = self.recurrent_kernel.unsqueeze(0)
        h0 = c0 = None
        if initial_state is not None:
            h0, c0 = initial_state
            h0 = h0.reshape(D, b, U).to(inputs.dtype) if h0 is not None else None
            c0 = c0.reshape(D, b, U).float() if c0 is not None else None
        y, hT, cT = F.qlstm(zx, R, lengths, h0, c0, reverse=self.go_backwards)
        if not self.return_sequences:
            # the last state of each direction, in the output's quaternion-concatenated column layout
            y = hT.view(D, b, 4, self.q_units).permute(1, 2, 0, 3).reshape(b, D * U)
        if not self.bidirectional:
            hT, cT = hT[0], cT[0]
        return [y, hT, cT] if self.return_state else y

    def compute_output_shape(self, input_shape):
        assert input_shape and len(input_shape) == 3
        width = self.directions * self.units
        out = (input_shape[0], input_shape[1], width) if self.return_sequences else (input_shape[0], width)
        if self.return_state:
            state = ((self.directions,) if self.bidirectional else ()) + (input_shape[0], self.units)
            return [out, state, state]
        return out

    def get_config(self):
        cfg = super(QuaternionLSTM, self).get_config()
        cfg.update(units=self.units, return_sequences=self.return_sequences, return_state=self.return_state,
                   go_backwards=self.go_backwards, bidirectional=self.bidirectional, unit_forget_bias=self.unit_forget_bias,
                   init_criterion=self.init_criterion, kernel_regularizer=regularizers.serialize(self.kernel_regularizer),
                   recurrent_regularizer=regularizers.serialize(self.recurrent_regularizer), seed=self.seed)
        return cfg
