"""TIMIT transducer (Graves 2012, "Sequence Transduction with Recurrent Neural Networks"): one of the three sequence encoders, a
quaternion LSTM prediction network over the label history and a joint network, trained with the transducer loss
(functional.rnnt_loss, include/qk_rnnt.h) in place of the CTC cost.  The reference has no such model.  Nobody has measured a phone
error rate with it."""
import torch

from .. import functional as Fq
from ..complexnn import QuaternionDense, QuaternionLSTM
from ..keras_like import Layer, initializers, regularizers
from ..layers import Dense, Dropout, _GradScale, label_error_rate, rnnt_batch_cost
from .interspeech_model import EvalResult

CLASSES = 62            # the 61 TIMIT phones and the blank, which is the last class and doubles as start-of-sequence
BLANK = CLASSES - 1


class SymbolEmbedding(Layer):
    """keras.layers.Embedding: (...,) int symbols -> (..., output_dim), a row of the (input_dim, output_dim) table each."""

    def __init__(self, input_dim, output_dim, embeddings_initializer='random_uniform', embeddings_regularizer=None, **kwargs):
        super(SymbolEmbedding, self).__init__(**kwargs)
        self.input_dim, self.output_dim = int(input_dim), int(output_dim)
        self.embeddings_initializer = initializers.get(embeddings_initializer)
        self.embeddings_regularizer = regularizers.get(embeddings_regularizer)

    def build(self, input_shape=None):
        self.add_weight('embeddings', (self.input_dim, self.output_dim), initializer=self.embeddings_initializer,
                        regularizer=self.embeddings_regularizer)
        self.built = True

    def call(self, inputs):
        return torch.nn.functional.embedding(inputs.long(), self.embeddings)

    def compute_output_shape(self, input_shape):
        return tuple(input_shape) + (self.output_dim,)

    def get_config(self):
        cfg = super(SymbolEmbedding, self).get_config()
        cfg.update(input_dim=self.input_dim, output_dim=self.output_dim,
                   embeddings_initializer=initializers.serialize(self.embeddings_initializer),
                   embeddings_regularizer=regularizers.serialize(self.embeddings_regularizer))
        return cfg


class TimitQTransducer(torch.nn.Module):
    """encoder: a TimitQLSTM, TimitQTransformer or TimitQConformer instance; only its features(x, input_length) -- (B, 4, F, T) ->
    (B, T, E) -- is used.  Its output layer `pred` stays unused: it is marked not trainable, so that it stays out of
    `[p for p in model.parameters() if p.requires_grad]`, and it is left out of regularization_loss.

    Prediction network: SymbolEmbedding(62, pred_units) -- blank is the start-of-sequence symbol -- then `pred_layers`
    unidirectional QuaternionLSTM(pred_units) over [blank, l_1 .. l_U] with lengths = label_length + 1 (Dropout in front of every
    layer).  Position u of its output is conditioned on the first u labels.

    Joint: QuaternionDense(joint_units) on the encoder output, QuaternionDense(joint_units, use_bias=False) on the prediction
    output, a broadcast add and tanh in torch ops, then a linear real Dense(62): logits (B, T, Lmax + 1, 62), unnormalised -- the
    loss kernel fuses the log-softmax.  The (B, T, Lmax + 1, joint_units) tensor is materialised."""

    def __init__(self, encoder, pred_units=256, pred_layers=1, joint_units=512, dropout=0.1, l2=0.0):
        super(TimitQTransducer, self).__init__()
        if not hasattr(encoder, 'features'):
            raise TypeError('TimitQTransducer: the encoder must have a features(x, input_length) method')
        if pred_units % 4 or joint_units % 4 or pred_units <= 0 or joint_units <= 0:
            raise ValueError('TimitQTransducer: pred_units and joint_units must be positive multiples of 4')
        if pred_layers < 1:
            raise ValueError('TimitQTransducer: pred_layers must be >= 1')
        reg = regularizers.l2(l2) if l2 else None
        self.encoder = encoder
        for m in encoder.pred.modules():             # the CTC output layer: frozen whether or not it has been built yet
            if isinstance(m, Layer):
                m.trainable = False
        for p in encoder.pred.parameters():
            p.requires_grad_(False)
        self.pred_units, self.joint_units, self.rate = pred_units, joint_units, dropout
        self.embed = SymbolEmbedding(CLASSES, pred_units, name='pred_embed')
        self.pred_rnn = torch.nn.ModuleList([QuaternionLSTM(pred_units, return_state=True, kernel_regularizer=reg,
                                                            recurrent_regularizer=reg, seed=4242 + 16 * i, name='pred_qlstm%d' % i)
                                             for i in range(pred_layers)])
        self.drop = Dropout(dropout)
        self.joint_enc = QuaternionDense(joint_units, kernel_regularizer=reg, seed=4301, name='joint_enc')
        self.joint_pred = QuaternionDense(joint_units, use_bias=False, kernel_regularizer=reg, seed=4302, name='joint_pred')
        self.joint_out = Dense(CLASSES, kernel_regularizer=reg, use_bias=True, bias_initializer='zeros',
                               kernel_initializer='random_uniform', name='joint_out')

    # ---- the three networks ------------------------------------------------------------------------------------------------------------
    def ensure_built(self, enc_width, device):
        """Create the weights of the prediction network and of the joint for an encoder output `enc_width` wide (the encoder builds
        its own on its first call)."""
        self.embed.ensure_built((None,), device)
        for layer in self.pred_rnn:
            layer.ensure_built((None, None, self.pred_units), device)
        self.joint_enc.ensure_built((None, enc_width), device)
        self.joint_pred.ensure_built((None, self.pred_units), device)
        self.joint_out.ensure_built((None, self.joint_units), device)

    def _embed(self, tokens, dtype):
        self.embed.ensure_built(tokens.shape, tokens.device)
        return self.embed.call(tokens).to(dtype)

    def predict(self, labels, label_length, dtype=torch.float32):
        """(B, Lmax) labels -> (B, Lmax + 1, pred_units): the prediction network over [blank, l_1 .. l_U].  Padding labels are
        replaced by blank before the lookup, so what they hold reaches nothing."""
        b, lmax = labels.shape
        ll = label_length.reshape(-1).to(labels.device).clamp(0, lmax)
        lab = torch.where(torch.arange(lmax, device=labels.device)[None, :] < ll[:, None], labels.long().clamp(0, CLASSES - 1),
                          torch.full((), BLANK, dtype=torch.long, device=labels.device))
        tokens = torch.cat([torch.full((b, 1), BLANK, dtype=torch.long, device=labels.device), lab], dim=1)
        o = self._embed(tokens, dtype)
        lengths = (ll + 1).to(torch.int32)
        for layer in self.pred_rnn:
            o = layer(self.drop(o), lengths=lengths)[0]
        return o

    def predict_step(self, tokens, state=None, dtype=torch.float32):
        """One step of the prediction network: tokens (B,) int, state = [(h, c)] per layer, or None for the zero state (`dtype` is
        then the activations' type).  Returns (output (B, pred_units), new state)."""
        dtype = state[0][0].dtype if state is not None else dtype
        o = self._embed(tokens.reshape(-1, 1), dtype)
        new = []
        for i, layer in enumerate(self.pred_rnn):
            o, h, c = layer(o, initial_state=state[i] if state is not None else None)
            new.append((h, c))
        return o[:, 0], new

    def joint_logits(self, enc, pred):
        """enc (B, T, E), pred (B, U1, pred_units) -> unnormalised logits (B, T, U1, 62)."""
        b, t, e = enc.shape
        u1 = pred.shape[1]
        fe = self.joint_enc(enc.reshape(b * t, e)).view(b, t, 1, self.joint_units)
        fp = self.joint_pred(pred.reshape(b * u1, pred.shape[2])).view(b, 1, u1, self.joint_units)
        return self.joint_out(torch.tanh(fe + fp))

    def forward(self, x, input_length=None):
        """Logits (B, T, 1, 62) against the empty label history: what the first decoding step of every frame sees (and the call that
        builds every weight, like Keras' build-on-first-call)."""
        enc = self.encoder.features(x, input_length)
        labels = torch.zeros((enc.shape[0], 0), dtype=torch.long, device=enc.device)
        pred = self.predict(labels, torch.zeros(enc.shape[0], dtype=torch.int32, device=enc.device), enc.dtype)
        return self.joint_logits(enc, pred)

    # ---- training -------------------------------------------------------------------------------------------------------------------------
    def transducer_loss(self, x, labels, input_length, label_length, loss_scale=1.0):
        """Per-sample transducer cost (B, 1).  loss_scale multiplies the gradient sent back through the network, not the cost."""
        enc = self.encoder.features(x, input_length)
        pred = self.predict(labels.to(enc.device), label_length, enc.dtype)
        logits = self.joint_logits(enc, pred)
        return rnnt_batch_cost(logits, labels, input_length, label_length, loss_scale=loss_scale)

    def regularization_loss(self):
        """Sum of the kernel regularisers of every layer in use (the encoder's unused output layer is left out)."""
        unused = set(id(m) for m in self.encoder.pred.modules())
        terms = [t for m in self.modules() if isinstance(m, Layer) and id(m) not in unused for t in m.regularization_losses()]
        if not terms:
            return next(self.parameters()).new_zeros(())
        return torch.stack([t.float() for t in terms]).sum()

    def training_loss(self, x, labels, input_length, label_length, loss_scale=1.0):
        """Mean transducer cost over the batch + the regularisation terms; loss_scale changes gradients only, and the regulariser
        goes through the same identity-forward / scaled-backward node (TimitQCNN.training_loss)."""
        reg = self.regularization_loss()
        if isinstance(loss_scale, torch.Tensor):
            loss_scale = Fq.loss_scale_arg(loss_scale, x.device)
        if isinstance(loss_scale, torch.Tensor) or loss_scale != 1.0:
            reg = _GradScale.apply(reg, loss_scale)
        return self.transducer_loss(x, labels, input_length, label_length, loss_scale=loss_scale).mean() + reg

    # ---- decoding and scoring -----------------------------------------------------------------------------------------------------------
    def _inference(self, fn):
        was = self.training
        self.train(False)
        try:
            with torch.no_grad():
                return fn()
        finally:
            self.train(was)

    def joint_step(self, fe_t, g):
        """log-softmax (B, 62) float32 of one frame's projected encoder output fe_t (B, joint_units) and the prediction outputs g (B,
        pred_units): the joint of decode()."""
        return torch.log_softmax(self.joint_out(torch.tanh(fe_t + self.joint_pred(g))).float(), dim=-1)

    @staticmethod
    def lowest_argmax(lsm):
        """argmax over the last axis, the lowest index on ties."""
        idx = torch.arange(lsm.shape[-1], device=lsm.device).expand_as(lsm)
        top = lsm.max(dim=-1, keepdim=True).values
        return torch.where(lsm == top, idx, torch.full_like(idx, lsm.shape[-1])).min(dim=-1).values

    def _greedy(self, x, input_length, max_symbols):
        if max_symbols < 1:
            raise ValueError('decode: max_symbols must be >= 1')
        enc = self.encoder.features(x, input_length)
        b, t_max, e = enc.shape
        dev = enc.device
        il = (input_length.reshape(-1).to(dev) if input_length is not None else torch.full((b,), t_max, device=dev)).long().clamp(0, t_max)
        fe = self.joint_enc(enc.reshape(b * t_max, e)).view(b, t_max, self.joint_units)
        g, state = self.predict_step(torch.full((b,), BLANK, dtype=torch.long, device=dev), dtype=enc.dtype)
        width = t_max * max_symbols
        out = torch.full((b, width + 1), -1, dtype=torch.long, device=dev)          # (column `width` takes the writes of rows that emit nothing)
        n = torch.zeros(b, dtype=torch.long, device=dev)
        logp = torch.zeros(b, dtype=torch.float32, device=dev)
        blank = torch.full((), BLANK, dtype=torch.long, device=dev)
        for t in range(t_max):
            live = il > t
            for _ in range(max_symbols):
                lsm = self.joint_step(fe[:, t], g)
                sym = self.lowest_argmax(lsm)
                logp = logp + torch.where(live, lsm.gather(1, sym[:, None])[:, 0], torch.zeros((), device=dev))
                emit = live & (sym != BLANK)
                out.scatter_(1, torch.where(emit, n, torch.full_like(n, width))[:, None], torch.where(emit, sym, -torch.ones_like(sym))[:, None])
                n = n + emit.long()
                g2, state2 = self.predict_step(torch.where(emit, sym, blank), state)
                g = torch.where(emit[:, None], g2, g)
                state = [(torch.where(emit[:, None], h2, h), torch.where(emit[:, None], c2, c)) for (h, c), (h2, c2) in zip(state, state2)]
                live = emit                          # a row that drew blank has finished this frame
        return out[:, :width], n, logp

    def decode(self, x, input_length=None, max_symbols=4):
        """Greedy time-synchronous transducer decode of the eval-mode model: for every frame, up to max_symbols times, the argmax
        (lowest index on ties) of the joint of the frame and each row's prediction state; a non-blank symbol is appended and
        advances that row's prediction network, a blank moves the row to the next frame.  Both loops have fixed trip counts and
        no host read; the one read is of the longest decode, which trims the result.  Returns ([decoded (B, L) int64, -1-padded],
        log_prob (B, 1)): the form of layers.ctc_decode; log_prob is the sum of the chosen symbols' log-softmax values, blanks
        included.  A frame that uses up max_symbols moves on WITHOUT a blank having been drawn, so log_prob is the log-probability
        of a complete alignment of the decode only for a row none of whose frames ended that way."""
        def run():
            out, n, logp = self._greedy(x, input_length, max_symbols)
            longest = int(n.max()) if n.numel() else 0
            return [out[:, :longest]], logp.reshape(-1, 1)
        return self._inference(run)

    def transcribe(self, wave, lengths=None, max_symbols=4, **fbank_kw):
        """Waveforms to phone decodes on the device: features.quaternion_fbank(wave, lengths, **fbank_kw), then decode() with the
        frame counts as input_length."""
        from ..features import quaternion_fbank
        fbank_kw.setdefault('dtype', next(self.parameters()).dtype)
        x, frame_lengths = quaternion_fbank(wave, lengths, **fbank_kw)
        return self.decode(x, frame_lengths, max_symbols=max_symbols)

    def evaluate(self, x, labels, input_length, label_length, class_map=None, max_symbols=4):
        """One validation batch in eval mode: EvalResult(loss = mean transducer cost, errors / symbols = edit operations and
        reference labels summed over the batch, per = errors / symbols, decoded (B, L) int64 -1-padded, log_prob (B, 1)); the
        score is layers.label_error_rate of decode()."""
        def run():
            loss = self.transducer_loss(x, labels, input_length, label_length).mean()
            out, n, logp = self._greedy(x, input_length, max_symbols)
            decoded = out[:, :int(n.max()) if n.numel() else 0]
            errors, symbols, per = label_error_rate(decoded, None, labels, label_length, class_map)
            return EvalResult(loss, errors, symbols, per, decoded, logp.reshape(-1, 1))
        return self._inference(run)
