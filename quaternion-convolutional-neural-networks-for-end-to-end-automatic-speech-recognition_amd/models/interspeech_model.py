"""TIMIT quaternion CNN + CTC -- counterpart of models/interspeech_model.py:getTimitModel2D (:45-185).

Input (B, 4, 41, T) channels_first quaternion features; QuaternionConv2D(sf,(3,5),'same') ->
MaxPooling2D((1,3),'same') (frequency 41 -> 14, see layers.py) -> n/2 convs of sf filters ->
n/2 convs of 2*sf filters (PReLU + Dropout after each) -> Permute/reshape to (B, T, C*F) ->
3 x TimeDistributed(QuaternionDense(256)) -> TimeDistributed(Dense(62, softmax)) -> CTC.
`d` is the reference's attribute bag (num_layers, start_filter, act, aact, dropout, l2, model,
quat_init); only the quaternion branch (`d.model == 'quaternion'`) is built.
"""

import collections

import torch

from .. import _lib as L
from .. import functional as Fq
from ..complexnn import QuaternionConv2D, QuaternionDense
from ..keras_like import Layer, activations, regularizers
from ..layers import (Dense, Dropout, MaxPooling2D, PReLU, TimeDistributed, ctc_align, ctc_batch_cost, ctc_decode,
                      dense_softmax_ctc_mean, error_breakdown, label_error_rate)

# TimitQCNN.evaluate: mean CTC cost, edit operations and reference symbols summed over the batch, their ratio (the PER), the decodes
EvalResult = collections.namedtuple('EvalResult', 'loss errors symbols per decoded log_prob')


class TimitQCNN(torch.nn.Module):
    def __init__(self, num_layers=10, start_filter=32, act='relu', aact='none', dropout=0.0, l2=0.0,
                 quat_init='quaternion', internal_layout='channels_last', fuse_head=True, chain_convs=True):
        super(TimitQCNN, self).__init__()
        n, sf = num_layers, start_filter
        if aact != 'none':
            act = 'linear'                                   # interspeech_model.py:55-56
        reg = regularizers.l2(l2) if l2 else None
        conv_args = dict(activation=act, data_format='channels_first', padding='same', bias_initializer='zeros',
                         kernel_regularizer=reg, kernel_initializer=quat_init, use_bias=True,
                         internal_layout=internal_layout)
        dense_args = dict(activation=act, kernel_regularizer=reg, kernel_initializer='random_uniform',
                          bias_initializer='zeros', use_bias=True)
        self.aact, self.rate, self.act = aact, dropout, act
        self.fuse_head = fuse_head          # first TimeDistributed dense as an (F, 1) convolution (no transpose copy)
        self.chain_convs = (chain_convs and internal_layout == 'channels_last'      # body convs as one autograd node
                            and not L.dbg(L.QK_DBG_NO_CONV_CHAIN))
        self.conv = QuaternionConv2D(sf, (3, 5), name='conv', **conv_args)
        self.pool = MaxPooling2D(pool_size=(1, 3), padding='same')
        widths = [sf] * (n // 2) + [2 * sf] * (n // 2)
        self.convs = torch.nn.ModuleList([QuaternionConv2D(w, (3, 5), name='conv%d' % i, **conv_args)
                                          for i, w in enumerate(widths)])
        self.dense = torch.nn.ModuleList([TimeDistributed(QuaternionDense(256, **dense_args)) for _ in range(3)])
        n_act = 1 + len(widths) + 3
        self.prelu = torch.nn.ModuleList([PReLU(shared_axes=[1, 0]) for _ in range(n_act)]) if aact == 'prelu' else None
        self.drop = Dropout(dropout)
        self._drop_base = 0
        # optional: a one-element int32 device tensor (the step counter of functional.adam_step(step=<tensor>)) mixed into every
        # dropout seed ON THE DEVICE -- with it the launch arguments of a training step do not change from step to step, which
        # is what a captured graph needs (bench.ModelTrainStep.capture); fused post-op path only
        self.drop_step_dev = None
        self.pred = TimeDistributed(Dense(62, activation='softmax', kernel_regularizer=reg, use_bias=True,
                                          bias_initializer='zeros', kernel_initializer='random_uniform'))

    def _act(self, x, i):
        return self.prelu[i](x) if self.prelu is not None else x

    # ---- PReLU / Dropout fused into the kernels (functional.quaternion_conv_chain post-ops) ----------------------
    def _new_drop_base(self):
        """Base seed of this forward pass's dropout masks: drawn from torch's (CPU) generator, so `torch.manual_seed`
        controls the masks as it controls torch's own dropout, and mixed with the data-parallel rank -- replicas seeded
        alike must not drop the same units.  (The fused kernels apply round(rate * 256) / 256: 8 random bits per
        element, functional.PostOp.applied_rate; 0.3 -> 0.30078.)"""
        base = int(torch.randint(0, 2 ** 31 - 1, (1,)).item()) if (self.training and self.rate > 0) else 0
        rank = 0
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            rank = torch.distributed.get_rank()
        self._drop_base = (base ^ (rank * 0x9E3779B1)) & 0xffffffff

    def _post(self, k, out_shape, device, dropout=True):
        """Post-op spec of activation slot k behind a quaternion layer whose (channels_first / TimeDistributed) output
        shape is `out_shape`: the PReLU slopes of self.prelu[k] (built here: (1, F, 1) behind a convolution, i.e. one
        per position of spatial axis 0 of the channels-last buffer; (1, 1) behind a dense layer) -- or alpha=None, the
        relu form, for the aact='none' model -- and the dropout rate while training, with slot k's own mask seed."""
        rate = self.rate if (dropout and self.training) else 0.0
        seed = (self._drop_base + 7919 * (k + 1)) & 0xffffffff
        if self.prelu is None:
            return dict(alpha=None, alpha_axis=-1, rate=rate, seed=seed, seed_dev=self.drop_step_dev if rate > 0 else None)
        pl = self.prelu[k]
        pl.ensure_built(out_shape, device)
        axis = 0 if pl.alpha.numel() > 1 else -1
        return dict(alpha=pl.alpha, alpha_axis=axis, rate=rate, seed=seed, seed_dev=self.drop_step_dev if rate > 0 else None)

    def _link(self, layer, kernel, k, out_shape, device, fused, dropout=True, **geometry):
        """`layer` as a functional.quaternion_conv_chain link (kernel, bias, kwargs) in activation slot k, its weight given as the
        chain reads it: with the layer's own activation (linear / relu), or on the fused post-op path linear, followed by slot
        k's post-op (_post)."""
        if fused:
            return kernel, layer.bias, dict(geometry, activation=None, post=self._post(k, out_shape, device, dropout))
        return kernel, layer.bias, dict(geometry, activation=activations.serialize(layer.activation))

    def _head_kernel(self, shape, device, dtype, in_chain):
        """Permute((3,1,2)) + reshape + the first TimeDistributed(QuaternionDense) (interspeech_model.py:141-149) on the body
        output (B, C, F, T) of `shape` WITHOUT the 367 MB transpose copy: feature c*F + f of time step t is o[b, c, f, t], so the
        dense layer is a quaternion convolution with an (F, 1) 'valid' kernel over (F, T) -- same GEMM (K = F*C), same
        conj(W) (x) x table.  Returns (kernel, geometry kwargs).  In a chain (`in_chain`) on 16-bit device tensors with
        matrix-core widths the kernel is the dense PARAMETER itself, read in place as a channel-major kernel
        (functional.quaternion_conv_chain: dense_kernel_size) -- no permuted copy, no re-layout launches, no permuted gradient
        accumulation (8 small launches per step); otherwise the (F, 1, Cq, units) copy r[(cq*F + f), :] -> [f, 0, cq, :].
        Parameters stay the reference's (in_q, units)."""
        d0 = self.dense[0].layer
        b, c, f, t = shape
        d0.ensure_built((None, c * f), device)
        if (in_chain and dtype in (torch.bfloat16, torch.float16) and device.type == 'cuda' and (c // 4) % 32 == 0
                and (d0.r.shape[-1] // 4) % 32 == 0 and d0.r.is_contiguous()):
            return d0.r, dict(conj=True, dense_kernel_size=(f, 1))
        w = d0.r.view(c // 4, f, d0.r.shape[-1]).permute(1, 0, 2).unsqueeze(1).contiguous()
        return w, dict(strides=1, padding='valid', dilation_rate=1, conj=True)

    def forward(self, x):
        return self.pred(self.features(x))

    def features(self, x):
        """The (B, T, 256) output of the last TimeDistributed(QuaternionDense) -- what the softmax output layer `pred` reads.

        Which kernels run (fusable = chain_convs, a device input, fp32 / bf16 / fp16):
        * fused post-op path -- every activation (+ Dropout) is the epilogue of the kernel that produces it (aact == 'prelu':
          the kernel writes pre-activation and output, the next layer's backward-data applies the derivative; relu + dropout:
          the kernel writes only y = dropout(relu(pre)), the consumer's backward multiplies by (y > 0) / (1 - rate)).  Taken with
          PReLU when fusable and QK_DBG_NO_FUSED_PRELU is clear, and without PReLU when act == 'relu', training with rate > 0,
          fusable and QK_DBG_NO_FUSED_DROPOUT is clear.  The head is always a chain link, even with fuse_head=False;
          dense[1..2] join the chain in the relu form only, unless QK_DBG_NO_DENSE_IN_CHAIN.
        * otherwise the plain chain -- no PReLU, no active dropout, chain_convs, a device input, more than one body
          convolution, body activation linear or relu: the body convolutions as one autograd node,
          the head its last link when fuse_head and the head's activation is linear or relu.
        * otherwise layer by layer -- the head as the (F, 1) convolution on the kernel copy when fuse_head (device input),
          Permute + reshape when not.
        The first layer and its pooling run as one kernel per direction (conv_relu_pool without PReLU, conv_prelu_pool on the
        fused path) where the kernel takes the geometry and QK_DBG_NO_FUSED_FIRST is clear."""
        dev, relu_form = x.device, self.prelu is None
        fusable = self.chain_convs and x.is_cuda and x.dtype in (torch.bfloat16, torch.float16, torch.float32)
        if relu_form:
            fused = fusable and self.act == 'relu' and self.training and self.rate > 0 and not L.dbg(L.QK_DBG_NO_FUSED_DROPOUT)
        else:
            fused = fusable and not L.dbg(L.QK_DBG_NO_FUSED_PRELU)
        if fused:
            self._new_drop_base()

        # first layer: conv (3,5) 'same' + MaxPooling2D((1,3), 'same') over frequency (interspeech_model.py:97-103).  The fused
        # kernels never write the 41-bin activation; they read a plain channels_first buffer (how the reference's callers hold
        # the features) plane by plane, and a channels-last buffer behind a channels_first view as it is.
        c, pl = self.conv, self.pool
        c.ensure_built(x.shape, dev)
        xl, lay = (x, 'channels_first') if x.is_contiguous() else (x.movedim(1, -1), 'channels_last')
        one_kernel = ((relu_form or fused) and x.is_cuda and x.dim() == 4 and c.padding == 'same' and c.strides == (1, 1)
                      and c.dilation_rate == (1, 1) and c.internal_layout == 'channels_last' and pl.pool_size == (1, 3)
                      and pl.strides == (1, 3) and pl.padding == 'same' and pl.data_format == 'channels_last'
                      and not L.dbg(L.QK_DBG_NO_FUSED_FIRST))
        if relu_form:
            if one_kernel and activations.serialize(c.activation) == 'relu' and Fq.conv_relu_pool_supported(xl, c.kernel, 3, lay):
                o = Fq.conv_relu_pool(xl, c.kernel, c.bias, 3, lay).movedim(-1, 1)
            else:
                o = pl(c(x))
        elif fused:
            po = self._post(0, c.compute_output_shape(tuple(x.shape)), dev, dropout=False)
            if one_kernel and Fq.conv_prelu_pool_supported(xl, c.kernel, po['alpha'], po['alpha_axis'], 3, lay):
                o = Fq.conv_prelu_pool(xl, c.kernel, c.bias, po['alpha'], po['alpha_axis'], 3, lay).movedim(-1, 1)
            else:
                o = pl(Fq.quaternion_conv(x, c.kernel, c.bias, strides=c.strides, padding=c.padding, data_format='channels_first',
                                          dilation_rate=c.dilation_rate, activation=None, post=po))
        else:
            o = pl(self.prelu[0](c(x)))

        # body: the n convolutions (interspeech_model.py:105-137), activation slots 1..n
        chain = fused or (self.chain_convs and x.is_cuda and relu_form and not (self.training and self.rate > 0)
                          and len(self.convs) > 1
                          and all(activations.serialize(cv.activation) in ('linear', 'relu') for cv in self.convs))
        shape, links, k = tuple(o.shape), [], 1
        for cv in self.convs:
            if chain:
                cv.ensure_built(shape, dev)
                shape = cv.compute_output_shape(shape)
                links.append(self._link(cv, cv.kernel, k, shape, dev, fused, strides=cv.strides, padding=cv.padding,
                                        dilation_rate=cv.dilation_rate))
            else:
                o = self.drop(self._act(cv(o), k))
            k += 1

        # head: Permute((3,1,2)) + reshape + the first TimeDistributed dense layer (interspeech_model.py:140-149)
        d0, first = self.dense[0].layer, 0           # first: the first dense layer still to run
        if fused or (chain and self.fuse_head and activations.serialize(d0.activation) in ('linear', 'relu')):
            kernel, geometry = self._head_kernel(shape, dev, o.dtype, in_chain=True)
            width = d0.r.shape[-1]
            links.append(self._link(d0, kernel, k, (shape[0], shape[3], width), dev, fused, **geometry))
            k, first = k + 1, 1
            if fused and relu_form and not L.dbg(L.QK_DBG_NO_DENSE_IN_CHAIN):
                # the second and third dense layers (interspeech_model.py:150-166) as 1 x 1 conj-convolution links of the same
                # chain: relu (+ dropout behind the second) in the producing kernel, its derivative in the consumer's backward
                for i in (1, 2):
                    dn = self.dense[i].layer
                    dn.ensure_built((None, width), dev)
                    width = dn.r.shape[-1]
                    links.append(self._link(dn, dn.r, k, (shape[0], shape[3], width), dev, fused, dropout=(i < 2)))
                    k, first = k + 1, first + 1
        if chain:
            y = Fq.quaternion_conv_chain(o.movedim(1, -1), links)        # channels-last (B, F, T, C); (B, 1, T, units) with the head
            o = y.reshape(y.shape[0], y.shape[2], y.shape[3]) if first else y.movedim(-1, 1)
        if first == 0 and self.fuse_head and o.is_cuda:
            b, t = o.shape[0], o.shape[3]
            kernel, _ = self._head_kernel(tuple(o.shape), dev, o.dtype, in_chain=False)
            name = activations.serialize(d0.activation)
            act = name if name in ('linear', 'relu') else 'linear'
            y = Fq.quaternion_conv(o, kernel, d0.bias, 1, 'valid', 'channels_first', 1, act, conj=True)
            if act != name:
                y = d0.activation(y)
            o = self.drop(self._act(y.reshape(b, d0.r.shape[-1], t).permute(0, 2, 1), k))     # (B, units, 1, T) -> (B, T, units)
            k, first = k + 1, 1
        elif first == 0:
            o = o.permute(0, 3, 1, 2)                        # Permute((3,1,2)): (B, T, C, F)
            o = o.reshape(o.shape[0], o.shape[1], o.shape[2] * o.shape[3])

        # dense tail: the TimeDistributed(QuaternionDense(256)) layers not run yet (interspeech_model.py:150-166)
        for i in range(first, len(self.dense)):
            if fused:                                        # the slot's post-op as its own pass (relu alone: the GEMM epilogue)
                dn, (b, t, w) = self.dense[i].layer, o.shape
                dn.ensure_built((None, w), dev)
                po = self._post(k, (b, t, dn.r.shape[-1]), dev, dropout=(i < 2))
                relu = relu_form and po['rate'] == 0.0
                o = Fq.quaternion_dense(o.reshape(b * t, w), dn.r, dn.bias, activation='relu' if relu else None).reshape(b, t, -1)
                if not relu:
                    o = Fq.prelu_dropout(o, po['alpha'], po['alpha_axis'], po['rate'], po['seed'])
            else:
                o = self._act(self.dense[i](o), k)
                if i < 2:
                    o = self.drop(o)
            k += 1
        return o

    def ctc_loss(self, x, labels, input_length, label_length, loss_scale=1.0):
        """The model output of the reference: K.ctc_batch_cost per sample, shape (B, 1) (interspeech_model.py:178).
        loss_scale (float16 training): the gradient sent back through the network is multiplied by it, the returned cost is
        not; divide it out in the optimiser (functional.adam_step(grad_scale=1 / (world * loss_scale)))."""
        return ctc_batch_cost(self(x), labels, input_length, label_length, loss_scale=loss_scale)

    def ctc_mean_loss(self, x, labels, input_length, label_length, loss_scale=1.0):
        """mean over the batch of ctc_loss(...): what training minimises (the reference compiles the model with
        `loss={'ctc': lambda y_true, y_pred: y_pred}`, i.e. the mean of the per-sample costs of interspeech_model.py:178).  Same value
        and gradients as `self.ctc_loss(...).mean()`; on the device the output layer, the CTC cost and the mean are ONE autograd node
        (layers.dense_softmax_ctc_mean: no framework launch between the CTC kernel and the output layer's backward)."""
        if not (x.is_cuda and x.dtype in (torch.bfloat16, torch.float16)):
            return self.ctc_loss(x, labels, input_length, label_length, loss_scale=loss_scale).mean()
        feats = self.features(x)
        dense = self.pred.layer
        dense.ensure_built((None, feats.shape[-1]), x.device)
        loss = dense_softmax_ctc_mean(feats, dense, labels, input_length, label_length, loss_scale)
        if loss is None:
            loss = ctc_batch_cost(self.pred(feats), labels, input_length, label_length, loss_scale=loss_scale).mean()
        return loss

    # ---- validation: decoding and phone error rate ------------------------------------------------------------------------------
    def _inference(self, fn):
        """fn() in inference mode: dropout off (no dropout-seed draw), no autograd graph, the module's training flag restored."""
        was = self.training
        self.train(False)
        try:
            with torch.no_grad():
                return fn()
        finally:
            self.train(was)

    def decode(self, x, input_length=None, greedy=True, beam_width=100, top_paths=1, merge_repeated=True, lm=None, lm_weight=0.5,
               insertion_bonus=0.0):
        """K.ctc_decode of the eval-mode posteriors self(x) (the reference's val_function output, interspeech_model.py:182-185):
        layers.ctc_decode's ([decoded_k (B, L_k) int64, -1-padded] * top_paths, log_prob).  The model keeps the T frames of its
        input through the body, so input_length defaults to T for every sample.  lm (a qcnn_amd.lm.NgramLM, greedy=False only)
        fuses a phone n-gram LM into the beam search; log_prob is then the fused score (layers.ctc_decode)."""
        if lm is not None and greedy:
            raise ValueError('decode: a language model needs the beam search (greedy=False)')
        def run():
            y = self(x)
            il = input_length if input_length is not None else torch.full((y.shape[0],), y.shape[1], dtype=torch.int32, device=y.device)
            return ctc_decode(y, il, greedy=greedy, beam_width=beam_width, top_paths=top_paths, merge_repeated=merge_repeated, lm=lm,
                              lm_weight=lm_weight, insertion_bonus=insertion_bonus)
        return self._inference(run)

    def align(self, x, labels, input_length=None, label_length=None):
        """Forced alignment of the transcripts `labels` (B, Lmax) to the eval-mode posteriors self(x): layers.ctc_align's
        AlignResult(path (B, T), starts (B, Lmax), ends (B, Lmax), score (B,)) -- which frames the model gives to which phone.
        input_length defaults to T for every sample, as in decode(); label_length defaults to Lmax for every sample."""
        def run():
            y = self(x)
            il = input_length if input_length is not None else torch.full((y.shape[0],), y.shape[1], dtype=torch.int32, device=y.device)
            ll = label_length if label_length is not None else torch.full((y.shape[0],), labels.shape[1], dtype=torch.int32,
                                                                          device=y.device)
            return ctc_align(y, labels, il, ll)
        return self._inference(run)

    def transcribe(self, wave, lengths=None, greedy=True, beam_width=100, top_paths=1, lm=None, lm_weight=0.5, insertion_bonus=0.0,
                   **fbank_kw):
        """Waveforms to phone decodes on the device: features.quaternion_fbank(wave, lengths, **fbank_kw) (the model's input, in the
        parameters' dtype unless fbank_kw gives `dtype`), then decode() with input_length = the frame counts (and the optional LM).
        Returns decode()'s ([decoded_k (B, L_k) int64, -1-padded] * top_paths, log_prob), in inference mode."""
        if lm is not None and greedy:
            raise ValueError('transcribe: a language model needs the beam search (greedy=False)')
        from ..features import quaternion_fbank
        fbank_kw.setdefault('dtype', next(self.parameters()).dtype)
        x, frame_lengths = quaternion_fbank(wave, lengths, **fbank_kw)
        return self.decode(x, frame_lengths, greedy=greedy, beam_width=beam_width, top_paths=top_paths, lm=lm, lm_weight=lm_weight,
                           insertion_bonus=insertion_bonus)

    def evaluate(self, x, labels, input_length, label_length, greedy=True, beam_width=100, class_map=None, lm=None, lm_weight=0.5,
                 insertion_bonus=0.0):
        """One validation batch from ONE eval-mode forward: EvalResult(loss = mean CTC cost (what ctc_mean_loss gives in eval mode),
        errors / symbols = edit operations and reference labels summed over the batch, per = errors / symbols, decoded = the best
        path (B, L) int64 -1-padded, log_prob).  class_map (62,) int folds classes before the edit distance (-1 drops one).  lm
        (greedy=False only) decodes with a fused phone n-gram LM; log_prob is then the fused score.  The counts are device
        tensors: nothing waits for the GPU except layers.ctc_decode's read of the decode lengths."""
        if lm is not None and greedy:
            raise ValueError('evaluate: a language model needs the beam search (greedy=False)')

        def run():
            y = self(x)
            loss = ctc_batch_cost(y, labels, input_length, label_length).mean()
            decoded, log_prob = ctc_decode(y, input_length, greedy=greedy, beam_width=beam_width, top_paths=1, lm=lm,
                                           lm_weight=lm_weight, insertion_bonus=insertion_bonus)
            errors, symbols, per = label_error_rate(decoded[0], None, labels, label_length, class_map)
            return EvalResult(loss, errors, symbols, per, decoded[0], log_prob)
        return self._inference(run)

    def error_breakdown(self, x, labels, input_length, label_length, greedy=True, beam_width=100, class_map=None, lm=None, lm_weight=0.5,
                        insertion_bonus=0.0, confusion=None):
        """evaluate()'s PER split into its parts, from one eval-mode forward: the decode of decode() scored by
        layers.error_breakdown -- ErrorBreakdown(correct, substitutions, deletions, insertions, symbols, per), device tensors
        summed over the batch; per equals evaluate(...).per.  confusion: a (K + 1, K + 1) int32 device tensor the aligned pairs are
        added to (K = 39 with the TIMIT class_map); zero it once and pass it for every batch."""
        if lm is not None and greedy:
            raise ValueError('error_breakdown: a language model needs the beam search (greedy=False)')

        def run():
            decoded, _ = ctc_decode(self(x), input_length, greedy=greedy, beam_width=beam_width, top_paths=1, lm=lm, lm_weight=lm_weight,
                                    insertion_bonus=insertion_bonus)
            return error_breakdown(decoded[0], None, labels, label_length, class_map, confusion=confusion)
        return self._inference(run)

    def regularization_loss(self):
        """Sum of the kernel regularisers (l2(d.l2) on every conv / dense kernel, interspeech_model.py:63,68,173):
        the term Keras adds to the compiled model's loss on top of the CTC cost."""
        terms = [t for m in self.modules() if isinstance(m, Layer) for t in m.regularization_losses()]
        if not terms:
            return next(self.parameters()).new_zeros(())
        return torch.stack([t.float() for t in terms]).sum()

    def training_loss(self, x, labels, input_length, label_length, loss_scale=1.0):
        """What training the reference model minimises: mean CTC cost over the batch (the usual
        `loss={'ctc': lambda y_true, y_pred: y_pred}` compile) + the regularisation terms.  loss_scale changes GRADIENTS only:
        the regulariser goes through the same identity-forward / scaled-backward node as the CTC cost, so that ONE grad_scale in
        the optimiser undoes both and the value returned (what gets logged) is the unscaled loss.  loss_scale is a number or a
        one-element float32 device tensor (training.GradGuard.loss_scale), here and in ctc_loss / ctc_mean_loss."""
        reg = self.regularization_loss()
        if isinstance(loss_scale, torch.Tensor):
            loss_scale = Fq.loss_scale_arg(loss_scale, x.device)
        if isinstance(loss_scale, torch.Tensor) or loss_scale != 1.0:
            from ..layers import _GradScale
            reg = _GradScale.apply(reg, loss_scale)
        return self.ctc_mean_loss(x, labels, input_length, label_length, loss_scale=loss_scale) + reg


class _RealConv2D(Layer):
    """keras Conv2D(filters, (3, 5), data_format='channels_first', padding='same') of the reference's `d.model == "real"`
    branch (interspeech_model.py:92-96,109-113,124-128): a stock real-valued layer, outside the quaternion hot path -- torch's
    own convolution with TensorFlow's 'same' rule (odd kernels: symmetric padding)."""

    def __init__(self, filters, kernel_size, activation=None, kernel_regularizer=None, **kwargs):
        super(_RealConv2D, self).__init__(**kwargs)
        from ..keras_like import activations, initializers
        self.filters, self.kernel_size = filters, tuple(kernel_size)
        self.activation = activations.get(activation)
        self.kernel_regularizer = regularizers.get(kernel_regularizer)
        self._init = initializers.get('random_uniform')
        self._zeros = initializers.get('zeros')

    def build(self, input_shape):
        self.add_weight('kernel', self.kernel_size + (input_shape[1], self.filters), initializer=self._init,
                        regularizer=self.kernel_regularizer)                 # Keras layout (kh, kw, in, out)
        self.add_weight('bias', (self.filters,), initializer=self._zeros)
        self.built = True

    def call(self, inputs):
        w = self.kernel.permute(3, 2, 0, 1).to(inputs.dtype)
        y = torch.nn.functional.conv2d(inputs, w, self.bias.to(inputs.dtype), padding=(self.kernel_size[0] // 2, self.kernel_size[1] // 2))
        return self.activation(y)

    def compute_output_shape(self, input_shape):
        return (input_shape[0], self.filters) + tuple(input_shape[2:])


class TimitRealCNN(torch.nn.Module):
    """The `d.model == "real"` branch of getTimitModel2D (interspeech_model.py:92-96,109-113,124-128,159-169): Conv2D stack
    on (B, 3, 41, T), the same frequency pooling, three TimeDistributed(Dense(1024)), Dense(62, softmax), CTC.  Stock
    real-valued layers throughout (torch ops): the comparison network of the paper, not part of the Hamilton hot path."""

    def __init__(self, num_layers=10, start_filter=32, act='relu', aact='none', dropout=0.0, l2=0.0):
        super(TimitRealCNN, self).__init__()
        n, sf = num_layers, start_filter
        if aact != 'none':
            act = 'linear'
        reg = regularizers.l2(l2) if l2 else None
        self.conv = _RealConv2D(sf, (3, 5), activation=act, kernel_regularizer=reg)
        self.pool = MaxPooling2D(pool_size=(1, 3), padding='same')
        widths = [sf] * (n // 2) + [2 * sf] * (n // 2)
        self.convs = torch.nn.ModuleList([_RealConv2D(w, (3, 5), activation=act, kernel_regularizer=reg) for w in widths])
        dense_args = dict(activation=act, kernel_regularizer=reg, kernel_initializer='random_uniform', bias_initializer='zeros', use_bias=True)
        self.dense = torch.nn.ModuleList([TimeDistributed(Dense(1024, **dense_args)) for _ in range(3)])
        self.prelu = torch.nn.ModuleList([PReLU(shared_axes=[1, 0]) for _ in range(1 + len(widths) + 3)]) if aact == 'prelu' else None
        self.drop = Dropout(dropout)
        self.pred = TimeDistributed(Dense(62, activation='softmax', kernel_regularizer=reg, use_bias=True,
                                          bias_initializer='zeros', kernel_initializer='random_uniform'))

    def _act(self, x, i):
        return self.prelu[i](x) if self.prelu is not None else x

    def forward(self, x):
        o = self.pool(self._act(self.conv(x), 0))
        k = 1
        for c in self.convs:
            o = self.drop(self._act(c(o), k))
            k += 1
        o = o.permute(0, 3, 1, 2)
        o = o.reshape(o.shape[0], o.shape[1], o.shape[2] * o.shape[3])
        for i, dl in enumerate(self.dense):
            o = self._act(dl(o), k)
            k += 1
            if i < 2:
                o = self.drop(o)
        return self.pred(o)

    def ctc_mean_loss(self, x, labels, input_length, label_length, loss_scale=1.0):
        """mean over the batch of ctc_loss(...): the composed output layer, CTC cost and mean (no fused node here)."""
        return self.ctc_loss(x, labels, input_length, label_length, loss_scale=loss_scale).mean()

    ctc_loss = TimitQCNN.ctc_loss
    regularization_loss = TimitQCNN.regularization_loss
    training_loss = TimitQCNN.training_loss


def getTimitModel2D(d):
    """(model, val_function) like the reference: `model(x)` gives the (B, T, 62) posteriors,
    `model.ctc_loss(...)` the CTC cost of interspeech_model.py:178, `model.training_loss(...)` that cost
    averaged over the batch plus the l2 terms Keras adds (d.l2); val_function(x) == model(x).
    d.model == 'quaternion' builds the engine's TimitQCNN on (B, 4, 41, T); d.model == 'real' the stock-layer comparison
    network on (B, 3, 41, T) (TimitRealCNN)."""
    kind = getattr(d, 'model', 'quaternion')
    if kind == 'real':
        m = TimitRealCNN(d.num_layers, d.start_filter, d.act, d.aact, d.dropout, getattr(d, 'l2', 0.0))
        return m, (lambda x: m(x))
    if kind != 'quaternion':
        raise ValueError("d.model must be 'quaternion' or 'real', got %r" % (kind,))
    m = TimitQCNN(d.num_layers, d.start_filter, d.act, d.aact, d.dropout, getattr(d, 'l2', 0.0),
                  getattr(d, 'quat_init', 'quaternion'))
    return m, (lambda x: m(x))
