"""torch.autograd bindings of the HIP Hamilton-product kernels (through the C-ABI only).

`quaternion_conv` / `quaternion_dense` compute what QuaternionConv.call
(complexnn/conv.py:288-345) and QuaternionDense.call (complexnn/dense.py:126-164) of the
reference compute, with the backward TF autodiff would produce -- on MI355X, from the
compact kernel, without materialising the 4x-expanded real kernel.

PyTorch is plumbing here: it owns the device buffers (caching allocator), supplies the
current HIP stream and chains the backward calls.  There is NO CPU or eager fallback:
a CPU tensor or a missing libqk_hip.so raises.
"""
import collections
import ctypes
import math

import numpy as np
import torch

from . import _lib as L
from ._shape import conv_output_length, normalize_tuple, tf_pads

_DTYPES = {torch.float32: L.QK_F32, torch.bfloat16: L.QK_BF16, torch.float16: L.QK_F16}
_PREP_CACHE_ON = not __import__('os').environ.get('QK_NO_PREP_CACHE')     # diagnostic: re-lay the 16-bit kernels out on every call
_PREP_PARAMS = __import__('weakref').WeakValueDictionary()   # id -> parameter that carries cached 16-bit re-layouts (_Call._ws)
_CAST_PARAMS = __import__('weakref').WeakValueDictionary()   # id -> tensor that carries a cached 16-bit cast (layers._cast_cached, _WeightedSumFn)
_PREP_WARNED = False


def invalidate_cached_kernels(params=None):
    """Drop every cached 16-bit image of the given parameters (default: of all parameters that carry one): the re-laid-out
    kernels of the quaternion layers and the 16-bit casts of the output layer / weighted_sum weights.

    The caches are keyed on the tensor's version counter, its flat buffer's version counter and its data pointer.  Every torch
    op, `FlatParams.adam_step`, `dp.broadcast_params` and `load_state_dict` bump one of them; a RAW write through `.data`
    (`p.data.copy_()`, `p.data.clamp_()`, an EMA / weight-averaging loop over `.data`, a c10d collective on `.data`) bumps none --
    call this afterwards (or use `with torch.no_grad(): p.copy_(...)`, which does bump the counter).  The next call of each
    layer rebuilds its image; returns the number of parameters touched."""
    if params is None:
        params = list(_PREP_PARAMS.values()) + list(_CAST_PARAMS.values())
    n = 0
    for p in params:
        hit = False
        for key in ('_qk_prep', '_qk_cast16', '_qk_cast'):
            if p.__dict__.pop(key, None) is not None:
                hit = True
        n += hit
    return n


def refresh_prepped_kernels(base=None):
    """Bring every cached 16-bit kernel re-layout up to date in ONE launch per device (qk_conv_prep_kernels): called by
    adam_step behind the update, so that the next training step's forward / backward calls find their workspace ready
    (desc.ws_has_kernel = 1) and launch nothing but the GEMM kernel -- 26 small launches per TIMIT step become one.
    base: restrict to the parameters that live in this flat buffer (or are this tensor).  Returns the number of jobs.
    A refresh that fails is not fatal (the optimiser step that called it has already happened): the device's entries
    are dropped from the cache and the next call of each layer re-lays its kernel out itself (ws_has_kernel = 0)."""
    per_dev = {}
    for p in list(_PREP_PARAMS.values()):
        cache = p.__dict__.get('_qk_prep')
        if not cache or not p.is_cuda:
            continue
        pbase = getattr(p, '_qk_flat_base', None)
        if base is not None and pbase is not base and p is not base:
            continue
        ver = (p._version, -1 if pbase is None else pbase._version)
        for key, ent in cache.items():
            if ent[0] == ver or ent[1] != p.data_ptr():
                continue
            per_dev.setdefault(p.device, []).append((p, key, ent, ver))
    total = 0
    for dev, jobs in per_dev.items():
        n = len(jobs)
        dp = (ctypes.POINTER(L.ConvDesc) * n)(*[ctypes.pointer(j[2][3][0]) for j in jobs])
        op_arr = (ctypes.c_int32 * n)(*[j[2][3][1] for j in jobs])
        w_arr = (ctypes.c_void_p * n)(*[j[0].data_ptr() for j in jobs])
        ws_arr = (ctypes.c_void_p * n)(*[j[2][2].data_ptr() for j in jobs])
        with torch.cuda.device(dev):
            rc = L.lib().qk_conv_prep_kernels(n, dp, op_arr, w_arr, ws_arr, _raw_stream(dev.index) if _raw_stream is not None
                                              else torch.cuda.current_stream(dev).cuda_stream)
        if rc != 0:
            # non-fatal (the optimiser step has already happened) but never silent: a sticky HIP fault or an argument bug would
            # otherwise show up only as 26 extra launches per step, or as a later unrelated failure
            msg = L.lib().qk_last_error()
            msg = msg.decode() if isinstance(msg, bytes) else str(msg)
            for p, key, ent, ver in jobs:
                p.__dict__.get('_qk_prep', {}).pop(key, None)
            if rc == L.QK_ERR_LAUNCH:
                raise RuntimeError('qk_conv_prep_kernels failed on %s: %s' % (dev, msg))
            global _PREP_WARNED
            if not _PREP_WARNED:
                _PREP_WARNED = True
                __import__('warnings').warn('qk_conv_prep_kernels refused the batched 16-bit kernel refresh on %s (rc %d: %s); the layers '
                                            're-lay their kernels out per call from now on' % (dev, rc, msg), RuntimeWarning)
            continue
        for p, key, ent, ver in jobs:
            ent[0] = ver
        total += n
    return total


def _require_device(t, what):
    if not t.is_cuda:
        raise RuntimeError('%s: got a CPU tensor. The quaternion layers run only on the MI355X HIP '
                           'path (libqk_hip.so); there is no CPU fallback.' % what)
    if t.dtype not in _DTYPES:
        raise TypeError('%s: unsupported dtype %s (float32, bfloat16, float16)' % (what, t.dtype))


def _ptr(t):
    return t.data_ptr() if t is not None else None      # argtypes are c_void_p: ints convert


# Host cost matters: the config-2 layer step is ~150 us of GPU time over 7 launches, so every
# microsecond of Python per launch shows up once a collective joins the step.
_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)


def _stream(t):
    if _raw_stream is not None:
        return _raw_stream(t.device.index)
    return torch.cuda.current_stream(t.device).cuda_stream


class _on_device(object):
    """torch.cuda.device(d) guard that is skipped when d is already the current device (the usual case)."""
    __slots__ = ('guard',)

    def __init__(self, dev):
        self.guard = None if torch.cuda.current_device() == dev.index else torch.cuda.device(dev)

    def __enter__(self):
        if self.guard is not None:
            self.guard.__enter__()

    def __exit__(self, *exc):
        if self.guard is not None:
            self.guard.__exit__(*exc)
        return False


class _Call(object):
    """One layer invocation: descriptor + the three C-ABI entry points it uses."""

    def __init__(self, desc, names, ws_fn, x_shape, y_shape, w_shape, relu):
        self.desc, self.names, self.ws_fn = desc, names, ws_fn
        self.x_shape, self.y_shape, self.w_shape, self.relu = x_shape, y_shape, w_shape, relu
        self.static_buffers = False      # True: keep workspaces (graph capture / bench loops)
        self._ws_cache = {}
        self._ws_bytes = {}              # the descriptor never changes after construction

    def _prep_job(self, op):
        """(conv descriptor, operation) that reproduces this call's kernel re-layout through qk_conv_prep_kernels."""
        d = self.desc
        if isinstance(d, L.DenseDesc):
            c = L.ConvDesc()
            c.rank, c.batch, c.cq, c.fq, c.dtype, c.conj, c.layout = 0, d.rows, d.in_q, d.q_units, d.dtype, 1, L.QK_CH_LAST
            for i in range(3):
                c.in_spatial[i] = c.out_spatial[i] = c.kernel[i] = c.stride[i] = c.dilation[i] = 1
        else:
            c = L.ConvDesc.from_buffer_copy(d)
        return c, (L.QK_OP_FWD if op == L.QK_OP_FWD else L.QK_OP_BWD_DATA)

    def _kernel_only_bytes(self, op):
        """Size of operation `op`'s workspace when it holds NOTHING but the re-laid-out 16-bit kernel (band layout + zero line,
        and for 16 / 32-channel layers the small-channel kernel's fragment layout behind it); 0 for fp32 and for
        channels_first descriptors (their workspace also carries re-laid-out operands).  The library is asked, never a formula
        restated here: the forward / backward-data figure IS the kernel-only size for such descriptors."""
        d = self.desc
        if d.dtype == L.QK_F32 or getattr(d, 'layout', L.QK_CH_LAST) != L.QK_CH_LAST:
            return 0
        cq, fq = (d.in_q, d.q_units) if isinstance(d, L.DenseDesc) else (d.cq, d.fq)
        if cq % 16 or fq % 16:
            return 0            # off the matrix-core path: the fp32-MFMA kernels never read the workspace -- nothing to cache or refresh
        kop = L.QK_OP_FWD if op == L.QK_OP_FWD else L.QK_OP_BWD_DATA
        n = self._ws_bytes.get(('k', kop))
        if n is None:
            n = self._ws_bytes[('k', kop)] = int(getattr(L.lib(), self.ws_fn)(ctypes.byref(self.desc), kop))
        return n

    def _prep_key(self, op):
        """Key of this call's cached re-layout on the parameter: (operation, conj, dtype) names the layout of a kernel read in its
        own (taps-major) order, whose taps, cq and fq follow from the parameter's shape.  A channel-major reading of the same
        parameter (the first TimeDistributed dense layer's weight read in place as an (F, 1) convolution kernel,
        qk_conv_desc_t.kernel_order) is a different layout of the same byte count, so its key also carries kernel_order, the taps,
        cq and fq -- with the three-part key alone, a model that ran that reading in training and the plain dense layer in
        evaluation handed each the other's layout."""
        d = self.desc
        key = ('f' if op == L.QK_OP_FWD else 't', int(d.conj) if hasattr(d, 'conj') else 1, int(d.dtype))
        if getattr(d, 'kernel_order', L.QK_KERNEL_TAPS_MAJOR) != L.QK_KERNEL_TAPS_MAJOR:
            key += (int(d.kernel_order), tuple(d.kernel), int(d.cq), int(d.fq))
        return key

    def _ws(self, op, like, wparam=None):
        """Workspace of operation `op`.  `wparam`: the PARAMETER the kernel argument is (a long-lived leaf tensor).  When the
        workspace holds only the kernel's 16-bit re-layout, it is kept ON the parameter together with the tensor version it
        was made from, and handed back with desc.ws_has_kernel = 1 as long as the weights have not changed -- the C side then
        skips the re-layout launch (26 launches per TIMIT training step).  Every in-place update bumps the version
        (torch ops do it themselves, adam_step through torch.autograd.graph.increment_version); a re-homed `.data` changes
        the pointer; a parameter re-homed into a dp.FlatParams buffer is also checked against THAT buffer's version (writes through
        the flat buffer -- the fused Adam, a broadcast -- do not touch the views' own counters); the cache dies with the parameter."""
        n = self._ws_bytes.get(op)
        if n is None:
            n = self._ws_bytes[op] = int(getattr(L.lib(), self.ws_fn)(ctypes.byref(self.desc), op))
        self.desc.ws_has_kernel = 0
        if n == 0:
            return None, 0
        if (wparam is not None and not self.static_buffers and n == self._kernel_only_bytes(op) and wparam.is_leaf
                and wparam.requires_grad and _PREP_CACHE_ON):
            key = self._prep_key(op)
            cache = wparam.__dict__.setdefault('_qk_prep', {})
            base = getattr(wparam, '_qk_flat_base', None)         # dp.FlatParams: the flat buffer this parameter is a view of --
            ver = (wparam._version, -1 if base is None else base._version)    # `.data` views do not share its version counter
            hit = cache.get(key)
            if hit is not None and hit[0] == ver and hit[1] == wparam.data_ptr() and hit[2].numel() == n \
                    and hit[2].device == like.device:
                self.desc.ws_has_kernel = 1
                return hit[2], n
            buf = torch.empty(n, dtype=torch.uint8, device=like.device)
            cache[key] = [ver, wparam.data_ptr(), buf, self._prep_job(op)]
            _PREP_PARAMS[id(wparam)] = wparam
            return buf, n
        if self.static_buffers:
            buf = self._ws_cache.get(op)
            if buf is None:
                buf = self._ws_cache[op] = torch.empty(n, dtype=torch.uint8, device=like.device)
            return buf, n
        return torch.empty(n, dtype=torch.uint8, device=like.device), n

    def fwd(self, x, w, bias, out=None, wparam=None):
        y = out if out is not None else torch.empty(self.y_shape, dtype=x.dtype, device=x.device)
        ws, n = self._ws(L.QK_OP_FWD, x, wparam)
        with _on_device(x.device):
            rc = getattr(L.lib(), self.names[0])(ctypes.byref(self.desc), _ptr(x), _ptr(w), _ptr(bias),
                                                 _ptr(y), _ptr(ws), n, _stream(x))
        L.check(rc, self.names[0])
        return y

    def bwd_data(self, dy, y, w, out=None, wparam=None):
        dx = out if out is not None else torch.empty(self.x_shape, dtype=dy.dtype, device=dy.device)
        ws, n = self._ws(L.QK_OP_BWD_DATA, dy, wparam)
        with _on_device(dy.device):
            rc = getattr(L.lib(), self.names[1])(ctypes.byref(self.desc), _ptr(dy), _ptr(y), _ptr(w),
                                                 _ptr(dx), _ptr(ws), n, _stream(dy))
        L.check(rc, self.names[1])
        return dx

    def bwd_weight(self, x, dy, y, has_bias, out=None, masked_dy_out=None, accumulate=False):
        """dw, db.  `masked_dy_out` (a tensor like dy) receives dy*(y>0) for RELU layers.
        accumulate=True adds into `out` instead of overwriting it (qk_*_bwd_weight_acc)."""
        if out is not None:
            dw, db = out
        else:
            dw = torch.empty(self.w_shape, dtype=torch.float32, device=x.device)
            db = torch.empty((self.w_shape[-1],), dtype=torch.float32, device=x.device) if has_bias else None
        ws, n = self._ws(L.QK_OP_BWD_WEIGHT, x)
        if masked_dy_out is not None:
            ws, n = masked_dy_out, masked_dy_out.numel() * masked_dy_out.element_size()
        with _on_device(x.device):
            name = self.names[2] + ('_acc' if accumulate else '')
            if accumulate and out is None:
                raise ValueError('accumulate=True needs the buffers to add into (out=)')
            rc = getattr(L.lib(), name)(ctypes.byref(self.desc), _ptr(x), _ptr(dy), _ptr(y),
                                        _ptr(dw), _ptr(db), _ptr(ws), n, _stream(x))
        L.check(rc, name)
        return dw, db


    def mask_bits_bytes(self):
        """Bytes of the bit-packed relu mask this layer's forward can write beside y (qk_conv_mask_bits_bytes), 0: it cannot."""
        return int(L.lib().qk_conv_mask_bits_bytes(ctypes.byref(self.desc)))

    def reads_mask_bits(self):
        """True when this layer's backward-data can read the bit-packed mask of its input (qk_conv_bwd_reads_mask_bits)."""
        return bool(L.lib().qk_conv_bwd_reads_mask_bits(ctypes.byref(self.desc)))

    def fwd_post(self, x, w, bias, post, wparam=None, bits_bytes=0):
        """(pre, y) = qk_conv_fwd_post: the LINEAR convolution and post(pre) (PReLU / dropout) from one launch.  The relu
        form of the post-op (post.alpha is None) writes y only: pre is None.  bits_bytes > 0 (relu form): returns
        (bits, y) instead, bits the uint8 bit-packed mask y > 0 (qk_conv_fwd_post_bits)."""
        pre = torch.empty(self.y_shape, dtype=x.dtype, device=x.device) if post.alpha is not None else None
        y = torch.empty(self.y_shape, dtype=x.dtype, device=x.device)
        ws, n = self._ws(L.QK_OP_FWD, x, wparam)
        if bits_bytes:
            bits = torch.empty(bits_bytes, dtype=torch.uint8, device=x.device)
            with _on_device(x.device):
                rc = L.lib().qk_conv_fwd_post_bits(ctypes.byref(self.desc), ctypes.byref(post.struct), _ptr(x), _ptr(w), _ptr(bias),
                                                   None, _ptr(y), _ptr(bits), _ptr(ws), n, _stream(x))
            L.check(rc, 'qk_conv_fwd_post_bits')
            return bits, y
        with _on_device(x.device):
            rc = L.lib().qk_conv_fwd_post(ctypes.byref(self.desc), ctypes.byref(post.struct), _ptr(x), _ptr(w), _ptr(bias),
                                          _ptr(pre), _ptr(y), _ptr(ws), n, _stream(x))
        L.check(rc, 'qk_conv_fwd_post')
        return pre, y

    def bwd_post(self, x, dy, w, has_bias, post_x, x_pre, dalpha_x, direct=None, wparam=None, x_bits=None):
        """Fused backward of a LINEAR layer whose input x = post_x(x_pre): returns (d x_pre, dw, db) and accumulates
        the slope gradient of post_x into dalpha_x (qk_conv_bwd_post).  direct = (dw, db) buffers to ADD into
        (QK_BWD_ACCUMULATE; the returned dw / db are then None).  Relu form of post_x: x_pre / dalpha_x are None, and
        x_bits (fwd_post's bit-packed mask of x) replaces reading x as the mask (qk_conv_bwd_post_bits)."""
        dx = torch.empty(self.x_shape, dtype=dy.dtype, device=dy.device)
        if direct is not None:
            dw, db = direct
        else:
            dw = torch.empty(self.w_shape, dtype=torch.float32, device=x.device)
            db = torch.empty((self.w_shape[-1],), dtype=torch.float32, device=x.device) if has_bias else None
        ws, n = self._ws(L.QK_OP_BWD, x, wparam)
        if x_bits is not None:
            with _on_device(x.device):
                rc = L.lib().qk_conv_bwd_post_bits(ctypes.byref(self.desc), _ptr(x), _ptr(x_bits), _ptr(dy), _ptr(w), _ptr(dx), _ptr(dw),
                                                   _ptr(db), ctypes.byref(post_x.struct), L.QK_BWD_ACCUMULATE if direct is not None else 0,
                                                   _ptr(ws), n, _stream(x))
            L.check(rc, 'qk_conv_bwd_post_bits')
            return (dx, None, None) if direct is not None else (dx, dw, db)
        with _on_device(x.device):
            rc = L.lib().qk_conv_bwd_post(ctypes.byref(self.desc), _ptr(x), _ptr(dy), _ptr(w), _ptr(dx), _ptr(dw), _ptr(db),
                                          ctypes.byref(post_x.struct), _ptr(x_pre), _ptr(dalpha_x),
                                          L.QK_BWD_ACCUMULATE if direct is not None else 0, _ptr(ws), n, _stream(x))
        L.check(rc, 'qk_conv_bwd_post')
        return (dx, None, None) if direct is not None else (dx, dw, db)

    def bwd(self, x, dy, y, w, has_bias, out=None, flags=0, wparam=None):
        """Fused backward (qk_*_bwd, or qk_*_bwd_chain with L.QK_BWD_* flags): returns (dx, dw, db)."""
        if out is not None:
            dx, dw, db = out
        else:
            dx = torch.empty(self.x_shape, dtype=dy.dtype, device=dy.device)
            dw = torch.empty(self.w_shape, dtype=torch.float32, device=x.device)
            db = torch.empty((self.w_shape[-1],), dtype=torch.float32, device=x.device) if has_bias else None
        ws, n = self._ws(L.QK_OP_BWD, x, wparam)
        name = self.names[1].replace('_bwd_data', '_bwd')
        with _on_device(x.device):
            if flags:
                name += '_chain'
                rc = getattr(L.lib(), name)(ctypes.byref(self.desc), _ptr(x), _ptr(dy), _ptr(y), _ptr(w), _ptr(dx),
                                            _ptr(dw), _ptr(db), int(flags), _ptr(ws), n, _stream(x))
            else:
                rc = getattr(L.lib(), name)(ctypes.byref(self.desc), _ptr(x), _ptr(dy), _ptr(y), _ptr(w), _ptr(dx),
                                            _ptr(dw), _ptr(db), _ptr(ws), n, _stream(x))
        L.check(rc, name)
        return dx, dw, db


class PostOp(object):
    """PReLU (+ Dropout) behind a quaternion layer (include/qk.h: qk_postop_t).  `alpha`: float32 device tensor, one
    slope (alpha_axis = -1) or one per position along spatial axis `alpha_axis` of the channels_last activation;
    `rate`: dropout rate (0 = off); `seed`: 32-bit seed of the counter-based mask (a new one every step);
    `seed_dev`: optional one-element int32 DEVICE tensor whose current value the kernels mix into the seed -- the step counter of
    `adam_step(step=<that tensor>)`: the launch arguments are then the same every step (graph replay) and the masks still change.
    alpha=None is the relu form y = dropout(relu(pre)): one output tensor, the backward reads only y.
    The rate the kernels apply is round(rate * 256) / 256 (8 random bits per element): `applied_rate`."""

    def __init__(self, alpha, alpha_axis=-1, rate=0.0, seed=0, seed_dev=None):
        if alpha is not None and (alpha.dtype != torch.float32 or not alpha.is_cuda):
            raise TypeError('PReLU slopes must be float32 device tensors')
        if seed_dev is not None and (seed_dev.dtype != torch.int32 or not seed_dev.is_cuda or seed_dev.numel() != 1):
            raise TypeError('seed_dev must be a one-element int32 device tensor (the training step counter of adam_step)')
        self.seed_dev = seed_dev                      # kept alive: the struct below holds its address
        if not 0.0 <= float(rate) < 1.0:
            raise ValueError('dropout rate must be in [0, 1), got %r' % (rate,))
        self.alpha, self.alpha_axis, self.rate, self.seed = alpha, int(alpha_axis), float(rate), int(seed) & 0xffffffff
        self.applied_rate = min(255, int(self.rate * 256.0 + 0.5)) / 256.0
        self.flat = alpha.detach().reshape(-1).contiguous() if alpha is not None else None
        self.struct = L.PostOp(self.alpha_axis if alpha is not None else -1, self.flat.numel() if alpha is not None else 0,
                               self.flat.data_ptr() if alpha is not None else None, self.rate, self.seed,
                               seed_dev.data_ptr() if seed_dev is not None else None)


def _tensor_desc(t):
    """ConvDesc fields the post-op entry points read, for a channels_last (N, *spatial, 4F) or (M, 4F) tensor."""
    d = L.ConvDesc()
    d.rank, d.batch, d.fq, d.dtype = t.dim() - 2, t.shape[0], t.shape[-1] // 4, _DTYPES[t.dtype]
    for i in range(3):
        d.out_spatial[i] = t.shape[1 + i] if i < t.dim() - 2 else 1
    return d


def postop_fwd(pre, post):
    y = torch.empty_like(pre)
    d = _tensor_desc(pre)
    with _on_device(pre.device):
        rc = L.lib().qk_postop_fwd(ctypes.byref(d), ctypes.byref(post.struct), _ptr(pre), _ptr(y), _stream(pre))
    L.check(rc, 'qk_postop_fwd')
    return y


def postop_bwd(pre, dy, post, dalpha):
    """d pre (returned) and the slope gradient (accumulated into the float32 buffer `dalpha`).  Relu form of the
    post-op: pass the forward OUTPUT y as `pre`, dalpha=None."""
    dpre = torch.empty_like(pre)
    d = _tensor_desc(pre)
    with _on_device(pre.device):
        rc = L.lib().qk_postop_bwd(ctypes.byref(d), ctypes.byref(post.struct), _ptr(pre), _ptr(dy), _ptr(dpre), _ptr(dalpha),
                                   _stream(pre))
    L.check(rc, 'qk_postop_bwd')
    return dpre


class _PostOpFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pre, alpha, post):
        ctx.post = post
        y = postop_fwd(pre, post)
        ctx.save_for_backward(pre if post.alpha is not None else y)      # relu form: the output is its own mask
        return y

    @staticmethod
    def backward(ctx, dy):
        pre, = ctx.saved_tensors
        post = ctx.post
        if post.alpha is None:
            return postop_bwd(pre, dy.contiguous(), post, None), None, None
        dalpha = torch.zeros(post.flat.numel(), dtype=torch.float32, device=pre.device)
        dpre = postop_bwd(pre, dy.contiguous(), post, dalpha)
        return dpre, dalpha.reshape(post.alpha.shape), None


def prelu_dropout(x, alpha, alpha_axis=-1, rate=0.0, seed=0):
    """y = dropout(prelu(x)) in ONE pass over a contiguous channels_last (N, *spatial, C) / (M, C) device tensor
    (keras PReLU + Dropout, interspeech_model.py:99-101,117-121); alpha: one slope or one per position along spatial
    axis `alpha_axis`.  The mask is a hash of (seed, element index): nothing is stored, the backward regenerates it."""
    _require_device(x, 'prelu_dropout')
    xc = x.contiguous()
    if xc.shape[-1] % (4 if xc.dtype == torch.float32 else 8) or xc.dim() < 2 or xc.dim() > 5:
        raise ValueError('prelu_dropout: unsupported shape %s' % (tuple(x.shape),))
    return _PostOpFn.apply(xc, alpha, PostOp(alpha, alpha_axis, rate, seed))


def relu_dropout(x, rate=0.0, seed=0):
    """y = dropout(relu(x)) in one pass (the relu form of prelu_dropout: no slopes; the backward reads y only)."""
    return prelu_dropout(x, None, -1, rate, seed)


def _direct_grad(w, b, want_w, want_b):
    """(dw, db) buffers to ACCUMULATE into, or None.  Parameters re-homed by dp.FlatParams carry `.grad` views of one
    flat, zeroed-after-the-step gradient buffer: the backward kernels add into them directly (qk_*_bwd_weight_acc /
    QK_BWD_ACCUMULATE) instead of filling a temporary that autograd then adds -- one memset and one elementwise pass
    less per parameter and step.  The caller returns None as these parameters' gradients and calls _grad_ready."""
    if not (want_w and getattr(w, '_qk_direct_grad', False) and w.grad is not None and w.grad.is_contiguous()
            and w.grad.dtype == torch.float32):
        return None
    if b is None:
        return w.grad, None
    if not (want_b and getattr(b, '_qk_direct_grad', False) and b.grad is not None and b.grad.is_contiguous()
            and b.grad.dtype == torch.float32):
        return None
    return w.grad, b.grad


def _grad_ready(*params):
    for p in params:
        cb = getattr(p, '_qk_grad_ready', None) if p is not None else None
        if cb is not None:
            cb(p)                         # dp.BucketedAllReduce counts its bucket down (autograd's hook will not fire)


class _HamiltonFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias, call):
        y = call.fwd(x, w, bias, wparam=w)
        ctx.call = call
        ctx.has_bias = bias is not None
        ctx.params = (w, bias)
        ctx.save_for_backward(x, w, y if call.relu else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        call = ctx.call
        dy = dy.contiguous()
        dx = dw = db = None
        want_w = ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2])
        direct = _direct_grad(ctx.params[0], ctx.params[1], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2])
        if ctx.needs_input_grad[0] and want_w:
            if direct is not None:
                dx = torch.empty(call.x_shape, dtype=dy.dtype, device=dy.device)
                call.bwd(x, dy, y, w, ctx.has_bias, out=(dx,) + direct, flags=L.QK_BWD_ACCUMULATE, wparam=ctx.params[0])
            else:
                dx, dw, db = call.bwd(x, dy, y, w, ctx.has_bias, wparam=ctx.params[0])        # fused: one pass over (dy, y)
        elif ctx.needs_input_grad[0]:
            dx = call.bwd_data(dy, y, w, wparam=ctx.params[0])
        elif want_w:
            if direct is not None:
                call.bwd_weight(x, dy, y, ctx.has_bias, out=direct, accumulate=True)
            else:
                dw, db = call.bwd_weight(x, dy, y, ctx.has_bias)
        if direct is not None and want_w:
            _grad_ready(*ctx.params)
        return dx, dw, db, None


def _act_code(activation):
    if activation in (None, 'linear'):
        return L.QK_ACT_LINEAR
    if activation == 'relu':
        return L.QK_ACT_RELU
    raise ValueError('fused activation must be None/"linear"/"relu", got %r' % (activation,))


def _check_weights(w, bias, n_out):
    if w.dtype != torch.float32 or (bias is not None and bias.dtype != torch.float32):
        raise TypeError('kernel / bias must be float32 (Keras floatx); activations may be 16-bit')
    if bias is not None and tuple(bias.shape) != (n_out,):
        raise ValueError('bias must have shape (%d,), got %s' % (n_out, tuple(bias.shape)))


def conv_call(x_shape, w_shape, dtype, rank, strides=1, padding='valid', layout='channels_last',
              dilation_rate=1, activation=None, use_bias=True, conj=False, kernel_order=0):
    """Descriptor for one conv call on a PHYSICAL layout (`layout` describes the buffer).  kernel_order =
    L.QK_KERNEL_CHANNEL_MAJOR: the kernel buffer lies as (cq, *kernel_size, 4 fq) -- a QuaternionDense weight read in place as
    the kernel of the equivalent convolution (include/qk.h); w_shape stays the logical (*kernel_size, cq, 4 fq)."""
    st = normalize_tuple(strides, rank, 'strides')
    dl = normalize_tuple(dilation_rate, rank, 'dilation_rate')
    if len(x_shape) != rank + 2 or len(w_shape) != rank + 2:
        raise ValueError('rank %d conv needs %d-D input and kernel' % (rank, rank + 2))
    if layout == 'channels_first':
        ci, sp = x_shape[1], tuple(x_shape[2:])
    else:
        ci, sp = x_shape[-1], tuple(x_shape[1:-1])
    cq, fq = w_shape[-2], w_shape[-1] // 4
    if ci != 4 * cq or w_shape[-1] != 4 * fq:
        raise ValueError('input channels %d / kernel shape %s are not quaternion-consistent'
                         % (ci, tuple(w_shape)))
    d = L.ConvDesc()
    d.rank, d.batch, d.cq, d.fq = rank, x_shape[0], cq, fq
    out_sp = []
    for i in range(3):
        if i < rank:
            k = w_shape[i]
            d.in_spatial[i], d.kernel[i], d.stride[i], d.dilation[i] = sp[i], k, st[i], dl[i]
            d.pad_lo[i] = tf_pads(sp[i], k, st[i], dl[i], padding)[0]
            d.out_spatial[i] = conv_output_length(sp[i], k, padding, st[i], dl[i])
            if d.out_spatial[i] <= 0:
                raise ValueError('convolution output would be empty on axis %d' % i)
            out_sp.append(d.out_spatial[i])
        else:
            d.in_spatial[i] = d.out_spatial[i] = d.kernel[i] = d.stride[i] = d.dilation[i] = 1
            d.pad_lo[i] = 0
    d.layout = L.QK_CH_FIRST if layout == 'channels_first' else L.QK_CH_LAST
    d.dtype = _DTYPES[dtype]
    d.activation = _act_code(activation)
    d.has_bias = int(bool(use_bias))
    d.conj = int(bool(conj))
    if layout == 'channels_first':
        y_shape = (x_shape[0], 4 * fq) + tuple(out_sp)
    else:
        y_shape = (x_shape[0],) + tuple(out_sp) + (4 * fq,)
    d.kernel_order = int(kernel_order)
    return _Call(d, ('qk_conv_fwd', 'qk_conv_bwd_data', 'qk_conv_bwd_weight'),
                 'qk_conv_workspace_bytes', tuple(x_shape), y_shape, tuple(w_shape),
                 d.activation == L.QK_ACT_RELU)


def dense_call(x_shape, w_shape, dtype, activation=None, use_bias=True):
    if len(x_shape) != 2 or len(w_shape) != 2:
        raise ValueError('quaternion dense needs 2-D input and kernel')
    in_q, units = w_shape
    if x_shape[1] != 4 * in_q or units % 4:
        raise ValueError('input width %d / kernel shape %s are not quaternion-consistent'
                         % (x_shape[1], tuple(w_shape)))
    d = L.DenseDesc()
    d.rows, d.in_q, d.q_units = x_shape[0], in_q, units // 4
    d.dtype = _DTYPES[dtype]
    d.activation = _act_code(activation)
    d.has_bias = int(bool(use_bias))
    return _Call(d, ('qk_dense_fwd', 'qk_dense_bwd_data', 'qk_dense_bwd_weight'),
                 'qk_dense_workspace_bytes', tuple(x_shape), (x_shape[0], units), tuple(w_shape),
                 d.activation == L.QK_ACT_RELU)


def quaternion_conv(x, kernel, bias=None, strides=1, padding='valid', data_format='channels_last',
                    dilation_rate=1, activation=None, conj=False, internal_layout='channels_last',
                    fold_small_cq=True, post=None):
    """y = act(W (x) x + b): Hamilton-product convolution of rank kernel.dim()-2.

    x       (N, *spatial, 4Cq) or (N, 4Cq, *spatial) -- component-planar channels (r|i|j|k)
    kernel  (*kernel_size, Cq, 4F) float32 compact kernel (conv.py:165, init.py:91)
    For data_format='channels_first' and internal_layout='channels_last' (default) the data is
    kept PHYSICALLY channels-last (a strided view with the logical channels_first shape is
    returned, torch.channels_last style): MFMA operands want the reduction axis contiguous.
    internal_layout='native' runs the channels_first buffers as they are.
    fold_small_cq: layers with 1-2 quaternion input channels whose input needs no gradient (the first
    layer of a network) are run as a 1x1 convolution on a tap-folded copy of x (qk_conv_fold_taps).
    post: dict(alpha=, alpha_axis=, rate=, seed=) -- PReLU (+ dropout) behind a LINEAR layer, fused into the
    kernel epilogues (see quaternion_conv_chain); alpha_axis counts the spatial axes of the layer output.
    """
    _require_device(x, 'quaternion_conv')
    rank = kernel.dim() - 2
    _check_weights(kernel, bias, kernel.shape[-1])
    ch_first = data_format == 'channels_first'
    taps, cq = int(math.prod(kernel.shape[:rank])), kernel.shape[-2]
    if x.shape[0] == 0:
        return _empty_batch(x, kernel, bias, rank, strides, padding, data_format, dilation_rate)
    if post is not None and internal_layout != 'channels_last':
        raise ValueError('a post-op needs internal_layout="channels_last"')
    if fold_small_cq and cq <= 2 and taps > 1 and taps * cq <= 64 and not x.requires_grad and not conj:
        return _folded_conv(x, kernel, bias, rank, strides, padding, data_format, dilation_rate, activation,
                            internal_layout, post)
    if post is not None:
        xl = x.movedim(1, -1) if ch_first else x
        y = quaternion_conv_chain(xl, [(kernel, bias, dict(strides=strides, padding=padding, dilation_rate=dilation_rate,
                                                           activation=activation, conj=conj, post=post))])
        return y.movedim(-1, 1) if ch_first else y
    if ch_first and internal_layout == 'channels_last':
        xp = x.movedim(1, -1).contiguous()
        layout = 'channels_last'
    else:
        xp = x.contiguous()
        layout = data_format
    call = conv_call(tuple(xp.shape), tuple(kernel.shape), xp.dtype, rank, strides, padding, layout,
                     dilation_rate, activation, bias is not None, conj)
    y = _HamiltonFn.apply(xp, kernel.contiguous(), bias, call)
    if ch_first and internal_layout == 'channels_last':
        y = y.movedim(-1, 1)
    return y


def _empty_batch(x, kernel, bias, rank, strides, padding, data_format, dilation_rate):
    """Zero samples: Keras returns an empty tensor of the right shape (and zero gradients); there is
    nothing to launch."""
    ch_first = data_format == 'channels_first'
    ks = tuple(kernel.shape[:rank])
    st, dl = normalize_tuple(strides, rank, 'strides'), normalize_tuple(dilation_rate, rank, 'dilation_rate')
    sp = x.shape[2:] if ch_first else x.shape[1:-1]
    out = tuple(conv_output_length(sp[i], ks[i], padding, st[i], dl[i]) for i in range(rank))
    shape = (0, kernel.shape[-1]) + out if ch_first else (0,) + out + (kernel.shape[-1],)
    y = torch.zeros(shape, dtype=x.dtype, device=x.device)
    tie = x.sum() * 0 + (kernel.sum() * 0).to(x.dtype)          # keeps autograd connected: zero gradients
    if bias is not None:
        tie = tie + (bias.sum() * 0).to(x.dtype)
    return y + tie


def _folded_conv(x, kernel, bias, rank, strides, padding, data_format, dilation_rate, activation, internal_layout,
                 post=None):
    ch_first = data_format == 'channels_first'
    xp = x.contiguous()
    taps, cq = int(math.prod(kernel.shape[:rank])), kernel.shape[-2]
    # folded channel count: a multiple of 8 (fp32 kernels) / of 32 (the 16-bit MFMA path) that holds every
    # (tap, channel) pair -- 32 for the 15-tap TIMIT layer, 64 for e.g. a 7x7 kernel on one channel
    gran = 32 if x.dtype != torch.float32 else 8
    cq2 = (taps * cq + gran - 1) // gran * gran
    call = conv_call(tuple(xp.shape), tuple(kernel.shape), xp.dtype, rank, strides, padding, data_format,
                     dilation_rate, None, False, False)
    d = call.desc
    out_sp = tuple(d.out_spatial[i] for i in range(rank))
    xcol = torch.empty((xp.shape[0],) + out_sp + (4 * cq2,), dtype=xp.dtype, device=xp.device)
    with _on_device(xp.device):
        rc = L.lib().qk_conv_fold_taps(ctypes.byref(d), _ptr(xp), _ptr(xcol), cq2, _stream(xp))
    L.check(rc, 'qk_conv_fold_taps')
    w2 = torch.nn.functional.pad(kernel.reshape(taps * cq, kernel.shape[-1]), (0, 0, 0, cq2 - taps * cq))
    w2 = w2.reshape((1,) * rank + (cq2, kernel.shape[-1]))
    y = quaternion_conv(xcol, w2, bias, 1, 'valid', 'channels_last', 1, activation, False, 'channels_last', False, post)
    return y.movedim(-1, 1) if ch_first else y


def quaternion_dense(x, kernel, bias=None, activation=None):
    """y = act(conj(W) (x) x + b) -- the table dense.py:139-143 builds (transpose of conv's)."""
    _require_device(x, 'quaternion_dense')
    _check_weights(kernel, bias, kernel.shape[-1])
    if x.shape[0] == 0:
        tie = x.sum() * 0 + (kernel.sum() * 0).to(x.dtype) + ((bias.sum() * 0).to(x.dtype) if bias is not None else 0)
        return torch.zeros((0, kernel.shape[-1]), dtype=x.dtype, device=x.device) + tie
    xp = x.contiguous()
    call = dense_call(tuple(xp.shape), tuple(kernel.shape), xp.dtype, activation, bias is not None)
    return _HamiltonFn.apply(xp, kernel.contiguous(), bias, call)


def adam_step(param, grad, m, v, step, lr=0.001, beta1=0.9, beta2=0.999, eps=1e-7, grad_scale=1.0, zero_grad=False,
              decay=None):
    """Fused Keras-Adam update of a flat float32 buffer (qk_adam_step); zero_grad=True also clears `grad`
    once it has been consumed (qk_adam_step_zero_grad), ready for accumulating backward calls.
    decay: per-element coefficients of the l2 kernel regularisers (dp.FlatParams.l2_decay): g += decay * param inside
    the kernel (qk_adam_step_l2) -- the gradient of the term Keras adds to the loss."""
    for t in (param, grad, m, v) + ((decay,) if decay is not None else ()):
        if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError('adam_step needs contiguous float32 device buffers')
    n = param.numel()
    if isinstance(step, torch.Tensor):
        # the step number lives on the device (qk_adam_step_dev): `step` holds the number of steps applied so far and is
        # incremented by the call -- no argument of the launch depends on the step (a captured graph replays correctly)
        if step.dtype != torch.int32 or not step.is_cuda or step.numel() != 1:
            raise TypeError('adam_step: a device-side step counter must be a one-element int32 device tensor')
        if decay is not None and decay.numel() != n:
            raise ValueError('decay must have one coefficient per parameter element')
        with _on_device(param.device):
            rc = L.lib().qk_adam_step_dev(_ptr(param), _ptr(grad), _ptr(m), _ptr(v), _ptr(decay), n, lr, beta1, beta2, eps,
                                          _ptr(step), grad_scale, int(bool(zero_grad)), _stream(param))
        L.check(rc, 'qk_adam_step_dev')
        torch.autograd.graph.increment_version(param)
        if _PREP_CACHE_ON:
            refresh_prepped_kernels(param)
        return
    with _on_device(param.device):
        if decay is not None:
            if decay.numel() != n:
                raise ValueError('decay must have one coefficient per parameter element')
            rc = L.lib().qk_adam_step_l2(_ptr(param), _ptr(grad), _ptr(m), _ptr(v), _ptr(decay), n, lr, beta1, beta2, eps,
                                         int(step), grad_scale, int(bool(zero_grad)), _stream(param))
        else:
            fn = L.lib().qk_adam_step_zero_grad if zero_grad else L.lib().qk_adam_step
            rc = fn(_ptr(param), _ptr(grad), _ptr(m), _ptr(v), n, lr, beta1, beta2, eps, int(step), grad_scale, _stream(param))
    L.check(rc, 'qk_adam_step')
    # the kernel wrote `param` behind torch's back: move its version counter (every view of a flat buffer shares it), so that
    # cached 16-bit re-layouts of the kernels (_Call._ws) are seen as stale
    torch.autograd.graph.increment_version(param)
    if _PREP_CACHE_ON:
        refresh_prepped_kernels(param)


def _flat_f32(what, *tensors):
    for t in tensors:
        if t is not None and (not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous()):
            raise RuntimeError('%s needs contiguous float32 device buffers' % what)


def _guard_state_ok(what, state, device):
    if (not isinstance(state, torch.Tensor) or state.dtype != torch.float32 or state.numel() != len(L.GRAD_GUARD_STATE)
            or not state.is_contiguous() or state.device != device):
        raise TypeError('%s: state must be the %d-element float32 device block of qk_grad_guard_state_t on the buffers\' device'
                        % (what, len(L.GRAD_GUARD_STATE)))


def grad_guard_reduce(grad, config, state, param=None, decay=None, grad_scale=1.0, workspace=None):
    """qk_grad_guard_reduce: the deterministic norm / non-finite reduction of the flat gradient and the step's decisions, written
    into `state` (the 8-element float32 device block that holds qk_grad_guard_state_t; training.GradGuard owns one).  config: a
    _lib.GradGuardConfig.  Nothing is read on the host."""
    _flat_f32('grad_guard_reduce', grad, param, decay)
    _guard_state_ok('grad_guard_reduce', state, grad.device)
    if (param is None) != (decay is None):
        raise ValueError('grad_guard_reduce: param and decay go together')
    n = grad.numel()
    if decay is not None and (decay.numel() != n or param.numel() != n):
        raise ValueError('param and decay must have one element per gradient element')
    need = int(L.lib().qk_grad_guard_workspace_bytes(n))
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=grad.device)
    with _on_device(grad.device):
        rc = L.lib().qk_grad_guard_reduce(_ptr(grad), _ptr(param), _ptr(decay), n, grad_scale, ctypes.byref(config), _ptr(state),
                                          _ptr(workspace), workspace.numel() * workspace.element_size(), _stream(grad))
    L.check(rc, 'qk_grad_guard_reduce')


def grad_norm(grad, param=None, decay=None, grad_scale=1.0):
    """(norm, nonfinite_count) of the flat float32 gradient as one-element DEVICE tensors (float32, int32): the global l2 norm of
    g = grad * grad_scale (+ decay * param), squares summed in float64 in a fixed order (bit-repeatable, no atomics), and the
    number of inf / NaN elements; the norm is +inf when there are any.  Two launches, no host read (qk_grad_guard_reduce with an
    inert configuration)."""
    _flat_f32('grad_norm', grad)
    state = torch.zeros(len(L.GRAD_GUARD_STATE), dtype=torch.float32, device=grad.device)
    state[0] = 1.0
    grad_guard_reduce(grad, L.GradGuardConfig(), state, param, decay, grad_scale)
    return state[4:5], state.view(torch.int32)[7:8]


def adam_step_guarded(param, grad, m, v, step, config, state, lr=0.001, beta1=0.9, beta2=0.999, eps=1e-7, zero_grad=False,
                      decay=None):
    """adam_step(step=<device tensor>) on the gradient grad_guard_reduce decided on (qk_adam_step_guarded): unscaled by
    state.last_unscale, clipped by state.last_coef and config.clipvalue, and not applied at all -- param, m, v and the step
    counter untouched, grad still cleared under zero_grad -- when state.last_skipped is set.  Run it behind grad_guard_reduce on
    the same buffers; training.GradGuard.step does both."""
    _flat_f32('adam_step_guarded', param, grad, m, v, decay)
    _guard_state_ok('adam_step_guarded', state, param.device)
    if not isinstance(step, torch.Tensor) or step.dtype != torch.int32 or not step.is_cuda or step.numel() != 1:
        raise TypeError('adam_step_guarded: the step counter must be a one-element int32 device tensor (a skipped step makes '
                        'the count data-dependent)')
    n = param.numel()
    if decay is not None and decay.numel() != n:
        raise ValueError('decay must have one coefficient per parameter element')
    with _on_device(param.device):
        rc = L.lib().qk_adam_step_guarded(_ptr(param), _ptr(grad), _ptr(m), _ptr(v), _ptr(decay), n, lr, beta1, beta2, eps,
                                          _ptr(step), int(bool(zero_grad)), ctypes.byref(config), _ptr(state), _stream(param))
    L.check(rc, 'qk_adam_step_guarded')
    torch.autograd.graph.increment_version(param)
    if _PREP_CACHE_ON:
        refresh_prepped_kernels(param)


def _opt_state_ok(what, state, device):
    if (not isinstance(state, torch.Tensor) or state.dtype != torch.float32 or state.numel() != len(L.OPT_STATE)
            or not state.is_contiguous() or state.device != device):
        raise TypeError('%s: opt_state must be the %d-element float32 device block of qk_opt_state_t on the buffers\' device'
                        % (what, len(L.OPT_STATE)))


def adam_step_sched(param, grad, m, v, step, schedule, opt_state, guard_config=None, guard_state=None, ema=None, ema_decay=0.0,
                    ema_warmup=True, beta1=0.9, beta2=0.999, eps=1e-7, grad_scale=1.0, zero_grad=False, decay=None):
    """adam_step(step=<device tensor>) / adam_step_guarded whose rate is the schedule's (qk_adam_step_sched, include/qk_opt.h):
    lr_eff = base_lr * w(t) * f(t) * opt_state.lr_scale, formed on the device from the step counter, so that no launch argument
    depends on the step.  schedule: a _lib.LRScheduleDesc; opt_state: the 8-element float32 device block that holds
    qk_opt_state_t (training.ScheduledAdam owns one).  guard_config / guard_state: both None (plain step, with grad_scale) or
    both given (the step grad_guard_reduce decided on; grad_scale must be 1).  ema: optional flat buffer that follows param with
    decay `ema_decay` (warmed up as TensorFlow's ExponentialMovingAverage does when ema_warmup).  A skipped step writes nothing
    but the cleared gradient.  Nothing is read on the host."""
    _flat_f32('adam_step_sched', param, grad, m, v, decay, ema)
    _opt_state_ok('adam_step_sched', opt_state, param.device)
    if (guard_config is None) != (guard_state is None):
        raise ValueError('adam_step_sched: guard_config and guard_state go together')
    if guard_state is not None:
        _guard_state_ok('adam_step_sched', guard_state, param.device)
        if grad_scale != 1.0:
            raise ValueError('adam_step_sched: grad_scale must be 1 with a guard (grad_guard_reduce already applied it)')
    if not isinstance(step, torch.Tensor) or step.dtype != torch.int32 or not step.is_cuda or step.numel() != 1:
        raise TypeError('adam_step_sched: the step counter must be a one-element int32 device tensor (the rate is a function of it)')
    n = param.numel()
    for name, t in (('grad', grad), ('m', m), ('v', v), ('decay', decay), ('ema', ema)):
        if t is not None and t.numel() != n:
            raise ValueError('adam_step_sched: %s must have one element per parameter element' % name)
    with _on_device(param.device):
        rc = L.lib().qk_adam_step_sched(_ptr(param), _ptr(grad), _ptr(m), _ptr(v), _ptr(decay), _ptr(ema), n, ctypes.byref(schedule),
                                        ema_decay, int(bool(ema_warmup)), beta1, beta2, eps, grad_scale, _ptr(step),
                                        int(bool(zero_grad)), ctypes.byref(guard_config) if guard_config is not None else None,
                                        _ptr(guard_state), _ptr(opt_state), _stream(param))
    L.check(rc, 'qk_adam_step_sched')
    torch.autograd.graph.increment_version(param)
    if _PREP_CACHE_ON:
        refresh_prepped_kernels(param)


def swap_(a, b):
    """Exchange the contents of two flat float32 device buffers in place, in one launch (qk_swap_f32); they must not overlap.
    Moves both version counters and brings the cached 16-bit kernel images of parameters living in either up to date."""
    _flat_f32('swap_', a, b)
    if a.numel() != b.numel() or a.device != b.device:
        raise ValueError('swap_: the buffers must have the same number of elements and live on one device')
    with _on_device(a.device):
        rc = L.lib().qk_swap_f32(_ptr(a), _ptr(b), a.numel(), _stream(a))
    L.check(rc, 'qk_swap_f32')
    for t in (a, b):
        torch.autograd.graph.increment_version(t)
        if _PREP_CACHE_ON:
            refresh_prepped_kernels(t)


class _MaxPoolCL(torch.autograd.Function):
    """qk_maxpool2d_fwd / _bwd on a channels_last buffer (N, H, W, C); windows == strides."""

    @staticmethod
    def forward(ctx, x, win, out_hw):
        n, h, w, c = x.shape
        d = L.PoolDesc(n, h, w, c, win[0], win[1], out_hw[0], out_hw[1], _DTYPES[x.dtype])
        y = torch.empty((n, out_hw[0], out_hw[1], c), dtype=x.dtype, device=x.device)
        with _on_device(x.device):
            rc = L.lib().qk_maxpool2d_fwd(ctypes.byref(d), _ptr(x), _ptr(y), _stream(x))
        L.check(rc, 'qk_maxpool2d_fwd')
        ctx.desc = d
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        with _on_device(x.device):
            rc = L.lib().qk_maxpool2d_bwd(ctypes.byref(ctx.desc), _ptr(x), _ptr(dy), _ptr(dx), _stream(x))
        L.check(rc, 'qk_maxpool2d_bwd')
        return dx, None, None


def maxpool2d_channels_last(x, window, out_hw):
    """Max pooling of a contiguous (N, H, W, C) device tensor with non-overlapping windows and
    high-side-only padding (see include/qk.h); returns (N, out_h, out_w, C)."""
    _require_device(x, 'maxpool2d_channels_last')
    return _MaxPoolCL.apply(x, tuple(window), tuple(out_hw))


def maxpool2d_supported(x, window, strides):
    vec = 4 if x.dtype == torch.float32 else 8
    return (x.is_cuda and x.dtype in _DTYPES and x.dim() == 4 and tuple(window) == tuple(strides)
            and x.shape[-1] % vec == 0 and x.numel() > 0 and x.numel() < 2 ** 31 and x.data_ptr() % 16 == 0)


class _ConvReluPoolFn(torch.autograd.Function):
    """qk_conv_relu_pool_fwd / _bwd: conv (3,5) 'same' + relu + max-pool over the first spatial axis as one launch per
    direction (the TIMIT model's first layer); the input gets no gradient."""

    @staticmethod
    def forward(ctx, x, w, bias, call, pool):
        n, h, wd = call.desc.batch, call.desc.in_spatial[0], call.desc.in_spatial[1]      # (x: (N, H, W, 4) or planes (N, 4, H, W))
        out = torch.empty((n, -(-h // pool), wd, w.shape[-1]), dtype=x.dtype, device=x.device)
        nb = int(L.lib().qk_conv_relu_pool_aux_bytes(ctypes.byref(call.desc), pool))
        keep = any(ctx.needs_input_grad[1:3])
        ctx.params = (w, bias)
        aux = torch.empty(nb, dtype=torch.uint8, device=x.device) if keep else None
        with _on_device(x.device):
            rc = L.lib().qk_conv_relu_pool_fwd(ctypes.byref(call.desc), pool, _ptr(x), _ptr(w), _ptr(bias), _ptr(out), _ptr(aux), _stream(x))
        L.check(rc, 'qk_conv_relu_pool_fwd')
        ctx.call, ctx.pool, ctx.has_bias = call, pool, bias is not None
        ctx.w_shape = tuple(w.shape)
        ctx.save_for_backward(x, aux)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, aux = ctx.saved_tensors
        dout = dout.contiguous()
        direct = _direct_grad(ctx.params[0], ctx.params[1], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2])
        if direct is not None:
            dw, db = direct
        else:
            dw = torch.empty(ctx.w_shape, dtype=torch.float32, device=x.device)
            db = torch.empty((ctx.w_shape[-1],), dtype=torch.float32, device=x.device) if ctx.has_bias else None
        with _on_device(x.device):
            rc = L.lib().qk_conv_relu_pool_bwd(ctypes.byref(ctx.call.desc), ctx.pool, _ptr(x), _ptr(dout), _ptr(aux), _ptr(dw), _ptr(db),
                                               L.QK_BWD_ACCUMULATE if direct is not None else 0, _stream(x))
        L.check(rc, 'qk_conv_relu_pool_bwd')
        if direct is not None:
            _grad_ready(*ctx.params)
            return None, None, None, None, None
        return None, dw, db, None, None


def _first_layer_call(x, kernel, activation, use_bias, x_layout):
    """Descriptor of the fused first layer; x_layout 'channels_last' = (N, H, W, 4), 'channels_first' = the four component
    planes (N, 4, H, W) read as they lie (include/qk.h: for these entry points desc.layout describes x only)."""
    if x_layout == 'channels_first':
        n, c, h, w = x.shape
        call = conv_call((n, h, w, c), tuple(kernel.shape), x.dtype, 2, 1, 'same', 'channels_last', 1, activation, use_bias, False)
        call.desc.layout = L.QK_CH_FIRST
        return call
    return conv_call(tuple(x.shape), tuple(kernel.shape), x.dtype, 2, 1, 'same', 'channels_last', 1, activation, use_bias, False)


def conv_relu_pool_supported(x, kernel, pool, x_layout='channels_last'):
    """True when relu(QuaternionConv2D(kernel, 'same')(x)) followed by MaxPooling over the first spatial axis (window =
    stride = pool, 'same') can run as the fused first-layer kernels: x a contiguous channels_last (N, H, W, 4) 16-bit
    device tensor that needs no gradient, kernel (3, 5, 1, 4F) with F % 8 == 0, pool == 3, and a height whose
    TensorFlow 'same' pooling pads on the high side only (H % 3 != 1: the kernel's windows start at row 0).  The
    answer is the C side's (qk_conv_relu_pool_aux_bytes is non-zero exactly for the geometries it takes), so the
    two predicates cannot drift apart."""
    ch_axis, h_axis = (1, 2) if x_layout == 'channels_first' else (-1, 1)
    if not (x.is_cuda and x.dtype in (torch.bfloat16, torch.float16) and x.dim() == 4 and x.shape[ch_axis] == 4 and not x.requires_grad
            and kernel.dim() == 4 and tuple(kernel.shape[:3]) == (3, 5, 1) and kernel.shape[-1] % 4 == 0 and x.shape[0] > 0):
        return False
    if tf_pads(x.shape[h_axis], pool, pool, 1, 'same')[0] != 0:
        return False
    try:
        call = _first_layer_call(x, kernel, 'relu', True, x_layout)
    except ValueError:
        return False
    return int(L.lib().qk_conv_relu_pool_aux_bytes(ctypes.byref(call.desc), pool)) > 0


def conv_relu_pool(x, kernel, bias=None, pool=3, x_layout='channels_last'):
    """(N, H, W, 4) -- or, with x_layout='channels_first', the component planes (N, 4, H, W) as the reference's model
    receives them -- -> channels_last (N, ceil(H / pool), W, 4F): the first TIMIT layer and its frequency pooling in one
    kernel (include/qk.h: qk_conv_relu_pool_*).  Check conv_relu_pool_supported first."""
    _require_device(x, 'conv_relu_pool')
    _check_weights(kernel, bias, kernel.shape[-1])
    xc = x.contiguous()
    call = _first_layer_call(xc, kernel, 'relu', bias is not None, x_layout)
    if not L.lib().qk_conv_relu_pool_aux_bytes(ctypes.byref(call.desc), pool):
        raise RuntimeError('conv_relu_pool: geometry outside the fused first-layer kernel')
    return _ConvReluPoolFn.apply(xc, kernel.contiguous(), bias, call, pool)


class _ConvPreluPoolFn(torch.autograd.Function):
    """qk_conv_prelu_pool_fwd / _bwd: linear conv (3,5) 'same' + PReLU (slope per row, or one) + max-pool over the first
    spatial axis as one launch per direction; the input gets no gradient."""

    @staticmethod
    def forward(ctx, x, w, bias, alpha, call, pool, post):
        n, h, wd = call.desc.batch, call.desc.in_spatial[0], call.desc.in_spatial[1]
        ctx.params = (w, bias)
        out = torch.empty((n, -(-h // pool), wd, w.shape[-1]), dtype=x.dtype, device=x.device)
        nb = int(L.lib().qk_conv_relu_pool_aux_bytes(ctypes.byref(call.desc), pool))
        keep = any(ctx.needs_input_grad[1:4])
        aux = torch.empty(nb, dtype=torch.uint8, device=x.device) if keep else None
        pre = torch.empty_like(out) if keep else None
        with _on_device(x.device):
            rc = L.lib().qk_conv_prelu_pool_fwd(ctypes.byref(call.desc), pool, ctypes.byref(post.struct), _ptr(x), _ptr(w), _ptr(bias),
                                                _ptr(out), _ptr(pre), _ptr(aux), _stream(x))
        L.check(rc, 'qk_conv_prelu_pool_fwd')
        ctx.call, ctx.pool, ctx.post, ctx.has_bias = call, pool, post, bias is not None
        ctx.w_shape = tuple(w.shape)
        ctx.save_for_backward(x, aux, pre)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, aux, pre = ctx.saved_tensors
        dout = dout.contiguous()
        post = ctx.post
        direct = _direct_grad(ctx.params[0], ctx.params[1], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2])
        if direct is not None:
            dw, db = direct
        else:
            dw = torch.empty(ctx.w_shape, dtype=torch.float32, device=x.device)
            db = torch.empty((ctx.w_shape[-1],), dtype=torch.float32, device=x.device) if ctx.has_bias else None
        da = torch.zeros(post.flat.numel(), dtype=torch.float32, device=x.device)
        with _on_device(x.device):
            rc = L.lib().qk_conv_prelu_pool_bwd(ctypes.byref(ctx.call.desc), ctx.pool, ctypes.byref(post.struct), _ptr(x), _ptr(dout),
                                                _ptr(pre), _ptr(aux), _ptr(dw), _ptr(db), _ptr(da),
                                                L.QK_BWD_ACCUMULATE if direct is not None else 0, _stream(x))
        L.check(rc, 'qk_conv_prelu_pool_bwd')
        if direct is not None:
            _grad_ready(*ctx.params)
            return None, None, None, da.reshape(post.alpha.shape), None, None, None
        return None, dw, db, da.reshape(post.alpha.shape), None, None, None


def conv_prelu_pool_supported(x, kernel, alpha, alpha_axis, pool, x_layout='channels_last'):
    """conv_relu_pool_supported for the PReLU form: float32 device slopes, one (alpha_axis -1) or one per position of
    the first spatial axis (alpha_axis 0, at most 64)."""
    n = alpha.numel()
    h = x.shape[2] if x_layout == 'channels_first' else x.shape[1]
    return (conv_relu_pool_supported(x, kernel, pool, x_layout) and alpha.is_cuda and alpha.dtype == torch.float32 and
            ((alpha_axis == -1 and n == 1) or (alpha_axis == 0 and n == h and n <= 64)))


def conv_prelu_pool(x, kernel, bias, alpha, alpha_axis=0, pool=3, x_layout='channels_last'):
    """(N, H, W, 4) [or planes (N, 4, H, W), x_layout='channels_first'] -> (N, ceil(H / pool), W, 4F): linear first layer +
    PReLU + frequency pooling in one kernel (include/qk.h: qk_conv_prelu_pool_*).  Check conv_prelu_pool_supported first."""
    _require_device(x, 'conv_prelu_pool')
    _check_weights(kernel, bias, kernel.shape[-1])
    xc = x.contiguous()
    call = _first_layer_call(xc, kernel, None, bias is not None, x_layout)
    post = PostOp(alpha, alpha_axis, 0.0, 0)
    return _ConvPreluPoolFn.apply(xc, kernel.contiguous(), bias, alpha, call, pool, post)


# Diagnostic tap (tests): when set to a callable it receives the list [x, y_1, ..., y_n] of every chain's activations
# as the forward produced them (tests/test_timit_parity.py compares the 16-bit gradients on the GPU's own relu masks).
chain_tap = None


class _ConvChainFn(torch.autograd.Function):
    """A run of quaternion convolutions applied back to back as ONE autograd node, so that the backward knows the
    structure.  Each layer ends in a fused relu (y_i = relu(W_i (x) y_{i-1} + b_i)), is linear, or carries a POST-OP
    (y_i = dropout(prelu(pre_i)), pre_i written beside y_i by the same launch):
      * relu: layer i+1's backward-data returns its input gradient already multiplied by (y_i > 0) (epilogue of the
        kernel, QK_BWD_MASK_DX) and layer i runs its backward without the mask and without reading y_i again
        (QK_BWD_DY_PREMASKED);
      * post-op: layer i+1's backward-data epilogue turns d y_i into d pre_i (dropout mask regenerated from the seed,
        PReLU derivative from pre_i) and accumulates d alpha_i (qk_conv_bwd_post); only the LAST layer's post-op needs
        a pass of its own (qk_postop_bwd).
    Gradients are identical to the layer-by-layer form."""

    @staticmethod
    def forward(ctx, x, calls, posts, *params):
        n = len(calls)
        ws, bs, alphas = params[:n], params[n:2 * n], params[2 * n:]
        acts, pres = [x], []
        # Bit-packed relu masks: link i -> i + 1 uses them when layer i has the relu-form post-op, its forward kernel can write the
        # bits and layer i + 1's backward-data can read them -- decided here, once, from both descriptors; pres[i] then holds the
        # bits (the relu form has no pre-activation to save).  The last link's own post-op has no consumer in the chain.
        no_bits = L.dbg(L.QK_DBG_NO_MASK_BITS)
        bits_bytes = [0] * n
        for i in range(n - 1):
            if posts[i] is not None and posts[i].alpha is None and not no_bits and calls[i + 1].reads_mask_bits():
                bits_bytes[i] = calls[i].mask_bits_bytes()
        for i, (call, w, b, post) in enumerate(zip(calls, ws, bs, posts)):
            if post is None:
                acts.append(call.fwd(acts[-1], w, b, wparam=w))
                pres.append(None)
            else:
                pre, y = call.fwd_post(acts[-1], w, b, post, wparam=w, bits_bytes=bits_bytes[i])
                acts.append(y)
                pres.append(pre)
        if chain_tap is not None:
            chain_tap(list(acts))
        ctx.calls, ctx.posts = calls, posts
        ctx.param_refs = (ws, bs)
        ctx.has_bias = [b is not None for b in bs]
        ctx.n_pre = [p is not None for p in pres]
        ctx.save_for_backward(*acts, *ws, *[p for p in pres if p is not None])
        return acts[-1]

    @staticmethod
    def backward(ctx, dy):
        calls, posts = ctx.calls, ctx.posts
        n = len(calls)
        saved = ctx.saved_tensors
        acts, ws = saved[:n + 1], saved[n + 1:2 * n + 1]
        it = iter(saved[2 * n + 1:])
        pres = [next(it) if has else None for has in ctx.n_pre]
        g = dy.contiguous()
        dws, dbs, das = [None] * n, [None] * n, [None] * n
        for i, post in enumerate(posts):
            if post is not None and post.alpha is not None:
                das[i] = torch.zeros(post.flat.numel(), dtype=torch.float32, device=g.device)
        if posts[n - 1] is not None:                      # the last post-op has no consumer inside the chain
            last = posts[n - 1]                           # (relu form: the output y is its own mask)
            g = postop_bwd(pres[n - 1] if last.alpha is not None else acts[n], g, last, das[n - 1])
        for i in range(n - 1, -1, -1):
            pw, pb = ctx.param_refs[0][i], ctx.param_refs[1][i]
            direct = _direct_grad(pw, pb, ctx.needs_input_grad[3 + i], ctx.has_bias[i] and ctx.needs_input_grad[3 + n + i])
            if i > 0 and posts[i - 1] is not None:
                relu_form = posts[i - 1].alpha is None                 # (then pres[i - 1] is the bit-packed mask of acts[i], or None)
                g, dws[i], dbs[i] = calls[i].bwd_post(acts[i], g, ws[i], ctx.has_bias[i], posts[i - 1], None if relu_form else pres[i - 1],
                                                      das[i - 1], direct=direct, wparam=pw, x_bits=pres[i - 1] if relu_form else None)
                if direct is not None:
                    _grad_ready(pw, pb)
                continue
            if i == 0 and not ctx.needs_input_grad[0]:
                # the chain's input needs no gradient (a first layer): backward-weight only.  (A relu layer whose dy
                # arrives masked is masked once more by this call -- idempotent.)
                if direct is not None:
                    calls[0].bwd_weight(acts[0], g, acts[1], ctx.has_bias[0], out=direct, accumulate=True)
                    _grad_ready(pw, pb)
                else:
                    dws[0], dbs[0] = calls[0].bwd_weight(acts[0], g, acts[1], ctx.has_bias[0])
                g = None
                continue
            flags = 0
            if i > 0 and calls[i - 1].relu:
                flags |= L.QK_BWD_MASK_DX
            if i < n - 1 and calls[i].relu:
                flags |= L.QK_BWD_DY_PREMASKED
            if direct is not None:
                dx = torch.empty(calls[i].x_shape, dtype=g.dtype, device=g.device)
                calls[i].bwd(acts[i], g, acts[i + 1], ws[i], ctx.has_bias[i], out=(dx,) + direct, flags=flags | L.QK_BWD_ACCUMULATE,
                             wparam=pw)
                _grad_ready(pw, pb)
                g = dx
            else:
                g, dws[i], dbs[i] = calls[i].bwd(acts[i], g, acts[i + 1], ws[i], ctx.has_bias[i], flags=flags, wparam=pw)
        das = [None if d is None else d.reshape(p.alpha.shape) for d, p in zip(das, posts)]      # (relu form: no slopes)
        dws = [None if d is None else d.reshape(w.shape) for d, w in zip(dws, ctx.param_refs[0])]   # (dense links: 2-D parameters)
        return (g, None, None) + tuple(dws) + tuple(dbs) + tuple(das)


def quaternion_conv_chain(x, layers):
    """Apply consecutive quaternion convolutions as one autograd node (see _ConvChainFn).
    `layers`: sequence of (kernel, bias, kwargs) with the keyword arguments of quaternion_conv
    (strides, padding, dilation_rate, activation ('relu' / 'linear' / None), conj) and optionally
    post=dict(alpha=<float32 tensor>, alpha_axis=-1|0|1|2, rate=<dropout rate>, seed=<int>): PReLU (+ dropout) behind
    a LINEAR layer (alpha=None: relu + dropout, the reference's aact='none' setting -- one output tensor per layer);
    x and every layer are channels_last here -- channels_first callers pass the channels-last view
    and move the axis back."""
    _require_device(x, 'quaternion_conv_chain')
    xp = x.contiguous()
    calls, ws, bs, posts, alphas = [], [], [], [], []
    shape = tuple(xp.shape)
    for kernel, bias, kw in layers:
        order = 0
        if kernel.dim() == 2 and kw.get('dense_kernel_size') is not None:
            # a QuaternionDense weight over the FLATTENED (channel, *kernel_size) axes of the feature map (the TIMIT model's first
            # TimeDistributed dense layer: row cq * F + f of the weight is tap f, channel cq of an (F, 1) 'valid' convolution,
            # interspeech_model.py:140-149): the parameter is read in place as a CHANNEL-MAJOR kernel (qk_conv_desc_t.kernel_order)
            # -- no permuted copy per step, cached 16-bit re-layout, kernel gradient straight into the parameter's own layout
            ksz = tuple(int(v) for v in kw['dense_kernel_size'])
            rank = len(ksz)
            taps = int(math.prod(ksz))
            if kernel.shape[0] % taps:
                raise ValueError('dense kernel rows %d are not a multiple of the %d taps' % (kernel.shape[0], taps))
            kw = dict(kw, conj=True, strides=1, padding='valid', dilation_rate=1)
            w_shape = ksz + (kernel.shape[0] // taps, kernel.shape[1])
            order = L.QK_KERNEL_CHANNEL_MAJOR
        elif kernel.dim() == 2:
            # a QuaternionDense weight (in_q, 4 * units): the layer applied to every position of the channels-last tensor is
            # the 1 x ... x 1 conj-convolution with that weight as its single tap (dense.py:139-143 builds the transposed
            # table).  The PARAMETER itself is passed on (same memory as the (1, ..., in_q, 4 units) kernel): its cached
            # 16-bit re-layout and the direct gradient writes keep working.
            rank = len(shape) - 2
            kw = dict(kw, conj=True, strides=1, padding='valid', dilation_rate=1)
            w_shape = (1,) * rank + tuple(kernel.shape)
        else:
            rank = kernel.dim() - 2
            w_shape = tuple(kernel.shape)
        _check_weights(kernel, bias, kernel.shape[-1])
        po = kw.get('post')
        if po is not None and kw.get('activation') not in (None, 'linear'):
            raise ValueError('a layer with a post-op must be linear (the post-op is its activation)')
        call = conv_call(shape, w_shape, xp.dtype, rank, kw.get('strides', 1), kw.get('padding', 'valid'),
                         'channels_last', kw.get('dilation_rate', 1), kw.get('activation'), bias is not None,
                         bool(kw.get('conj', False)), order)
        calls.append(call)
        ws.append(kernel.contiguous())
        bs.append(bias)
        posts.append(None if po is None else PostOp(po['alpha'], po.get('alpha_axis', -1), po.get('rate', 0.0), po.get('seed', 0), po.get('seed_dev')))
        alphas.append(None if po is None else po['alpha'])
        shape = tuple(call.y_shape)
    return _ConvChainFn.apply(xp, tuple(calls), tuple(posts), *ws, *bs, *alphas)


def softmax_rows_fwd(logits, bias, out_dtype):
    """softmax(logits + bias) over the last axis of an fp32 (rows, cols <= 64) device matrix, written in `out_dtype`
    (include/qk.h: qk_softmax_rows_fwd)."""
    _require_device(logits, 'softmax_rows_fwd')
    if logits.dtype != torch.float32 or logits.dim() != 2 or not logits.is_contiguous() or logits.shape[1] > 64:
        raise ValueError('softmax_rows_fwd: contiguous fp32 (rows, cols <= 64) logits')
    y = torch.empty(logits.shape, dtype=out_dtype, device=logits.device)
    with _on_device(logits.device):
        rc = L.lib().qk_softmax_rows_fwd(_DTYPES[out_dtype], logits.shape[0], logits.shape[1], _ptr(logits), _ptr(bias), _ptr(y), _stream(logits))
    L.check(rc, 'qk_softmax_rows_fwd')
    return y


def softmax_rows_bwd(y, dy, dbias=None):
    """d logits = y * (dy - <dy, y>) (returned, y's dtype); the bias gradient (column sums) is ADDED to the fp32 buffer `dbias`."""
    _require_device(y, 'softmax_rows_bwd')
    if dy.dtype != y.dtype or dy.shape != y.shape or dy.device != y.device or y.dim() != 2:
        raise ValueError('softmax_rows_bwd: dy must match y (2-D, same shape, dtype and device); got %s %s vs %s %s'
                         % (tuple(dy.shape), dy.dtype, tuple(y.shape), y.dtype))
    if dbias is not None and (dbias.dtype != torch.float32 or dbias.numel() != y.shape[1] or dbias.device != y.device or not dbias.is_contiguous()):
        raise ValueError('softmax_rows_bwd: dbias must be a contiguous fp32 device tensor with one entry per column')
    y, dy = y.contiguous(), dy.contiguous()           # raw pointers go to the kernel
    dl = torch.empty_like(y)
    with _on_device(y.device):
        rc = L.lib().qk_softmax_rows_bwd(_DTYPES[y.dtype], y.shape[0], y.shape[1], _ptr(y), _ptr(dy), _ptr(dl), _ptr(dbias), _stream(y))
    L.check(rc, 'qk_softmax_rows_bwd')
    return dl


def dense_softmax_supported(x, units):
    """True when qk_dense_softmax_fwd / _bwd take softmax(x @ kernel + bias) for this 16-bit (rows, in_dim) device matrix."""
    return (x.is_cuda and x.dim() == 2 and x.dtype in (torch.bfloat16, torch.float16) and x.is_contiguous()
            and bool(L.lib().qk_dense_softmax_supported(_DTYPES[x.dtype], x.shape[0], x.shape[1], int(units))))


def dense_softmax_fwd(x, kernel, bias):
    """y = softmax(x @ kernel + bias) in ONE launch (include/qk.h: qk_dense_softmax_fwd): x (rows, in_dim) 16-bit, kernel (in_dim, units)
    and bias (units) the fp32 master weights."""
    _require_device(x, 'dense_softmax_fwd')
    if kernel.dtype != torch.float32 or not kernel.is_contiguous() or kernel.dim() != 2 or kernel.shape[0] != x.shape[1] or kernel.device != x.device:
        raise ValueError('dense_softmax_fwd: kernel must be a contiguous fp32 (in_dim, units) device tensor')
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() != kernel.shape[1] or not bias.is_contiguous() or bias.device != x.device):
        raise ValueError('dense_softmax_fwd: bias must be a contiguous fp32 device tensor with one entry per unit')
    x = x.contiguous()
    y = torch.empty((x.shape[0], kernel.shape[1]), dtype=x.dtype, device=x.device)
    with _on_device(x.device):
        rc = L.lib().qk_dense_softmax_fwd(_DTYPES[x.dtype], x.shape[0], x.shape[1], kernel.shape[1], _ptr(x), _ptr(kernel), _ptr(bias), _ptr(y), _stream(x))
    L.check(rc, 'qk_dense_softmax_fwd')
    return y


def dense_softmax_bwd(x, kernel, y, dy, dkernel, dbias, dy_scale_dev=None, dy_scale=1.0):
    """dx (returned) of y = softmax(x @ kernel + bias); the kernel / bias gradients are ADDED to the fp32 buffers `dkernel` /
    `dbias` (None: not computed) -- qk_dense_softmax_bwd, one launch (+ the slab reduction).  dy enters multiplied by
    `dy_scale_dev` (a one-element fp32 DEVICE tensor or None) x `dy_scale` (a Python float)."""
    if dy_scale_dev is not None and (dy_scale_dev.dtype != torch.float32 or dy_scale_dev.numel() != 1 or dy_scale_dev.device != x.device):
        raise ValueError('dense_softmax_bwd: dy_scale_dev must be a one-element fp32 tensor on the device of x')
    _require_device(x, 'dense_softmax_bwd')
    if dy.dtype != y.dtype or dy.shape != y.shape or y.dtype != x.dtype or y.device != x.device or dy.device != x.device:
        raise ValueError('dense_softmax_bwd: y / dy must match each other and x in dtype and device')
    for name, t, n in (('dkernel', dkernel, kernel.numel()), ('dbias', dbias, kernel.shape[1])):
        if t is not None and (t.dtype != torch.float32 or t.numel() != n or not t.is_contiguous() or t.device != x.device):
            raise ValueError('dense_softmax_bwd: %s must be a contiguous fp32 device tensor of %d elements' % (name, n))
    x, y, dy = x.contiguous(), y.contiguous(), dy.contiguous()
    dx = torch.empty_like(x)
    with _on_device(x.device):
        ws, n = None, 0
        if dkernel is not None or dbias is not None:
            n = int(L.lib().qk_dense_softmax_bwd_workspace_bytes(_DTYPES[x.dtype], x.shape[0], x.shape[1], kernel.shape[1]))
            ws = torch.empty(n, dtype=torch.uint8, device=x.device)           # (the caching allocator hands the same block back every step)
        rc = L.lib().qk_dense_softmax_bwd(_DTYPES[x.dtype], x.shape[0], x.shape[1], kernel.shape[1], _ptr(x), _ptr(kernel), _ptr(y), _ptr(dy),
                                          _ptr(dx), _ptr(dkernel), _ptr(dbias), _ptr(dy_scale_dev), float(dy_scale), _ptr(ws), n, _stream(x))
    L.check(rc, 'qk_dense_softmax_bwd')
    return dx


class _WeightedSumFn(torch.autograd.Function):
    """sum(a * w) for a 16-bit / fp32 device tensor `a` and a CONSTANT fp32 weight tensor `w` as one launch (qk_weighted_sum);
    the backward hands back w in a's dtype (cast once, kept on the weight tensor)."""

    @staticmethod
    def forward(ctx, a, w):
        out = torch.zeros((), dtype=torch.float32, device=a.device)
        with _on_device(a.device):
            rc = L.lib().qk_weighted_sum(_DTYPES[a.dtype], a.numel(), _ptr(a), _ptr(w), _ptr(out), _stream(a))
        L.check(rc, 'qk_weighted_sum')
        cache = w.__dict__.setdefault('_qk_cast', {})
        _CAST_PARAMS[id(w)] = w
        hit = cache.get(a.dtype)
        ver = (w._version, w.data_ptr())
        if hit is None or hit[0] != ver:
            hit = cache[a.dtype] = (ver, w.to(a.dtype))
        ctx.wt = hit[1]
        ctx.a_shape = a.shape
        return out

    @staticmethod
    def backward(ctx, g):
        return (ctx.wt * g.to(ctx.wt.dtype)).reshape(ctx.a_shape), None          # (w may have a's element count in another shape)


def weighted_sum(a, w):
    """The linear functional sum(a * w) of a model output (the bench's stand-in loss), one launch forward, one backward."""
    _require_device(a, 'weighted_sum')
    if w.dtype != torch.float32 or w.numel() != a.numel() or w.requires_grad:
        raise ValueError('weighted_sum: w must be a constant fp32 tensor with as many elements as a')
    return _WeightedSumFn.apply(a.contiguous(), w.contiguous())


def _ctc_call(y_pred, labels, input_length, label_length, want_grad):
    """qk_ctc_batch_cost on a contiguous device y_pred (B, T, C): (cost (B,), d cost / d y_pred or None), one launch."""
    b, t, c = y_pred.shape
    lab = labels.to(device=y_pred.device, dtype=torch.int32).contiguous()
    il = input_length.reshape(-1).to(device=y_pred.device, dtype=torch.int32).contiguous()
    ll = label_length.reshape(-1).to(device=y_pred.device, dtype=torch.int32).contiguous()
    lmax = lab.shape[1] if lab.dim() == 2 else 0
    cost = torch.empty(b, dtype=torch.float32, device=y_pred.device)
    dpred = torch.empty_like(y_pred) if want_grad else None
    n = int(L.lib().qk_ctc_workspace_bytes(b, t, lmax))
    ws = torch.empty(n, dtype=torch.uint8, device=y_pred.device)
    with _on_device(y_pred.device):
        rc = L.lib().qk_ctc_batch_cost(_DTYPES[y_pred.dtype], b, t, c, _ptr(y_pred), _ptr(lab), lmax, _ptr(il), _ptr(ll), _ptr(cost),
                                       _ptr(dpred), _ptr(ws), n, _stream(y_pred))
    L.check(rc, 'qk_ctc_batch_cost')
    return cost, dpred


class _CtcFn(torch.autograd.Function):
    """qk_ctc_batch_cost: cost and d cost / d y_pred from one launch; the backward only scales the stored gradient."""

    @staticmethod
    def forward(ctx, y_pred, labels, input_length, label_length, loss_scale=1.0):
        cost, dpred = _ctc_call(y_pred, labels, input_length, label_length, ctx.needs_input_grad[0])
        ctx.save_for_backward(dpred)
        ctx.loss_scale = loss_scale if isinstance(loss_scale, torch.Tensor) else float(loss_scale)
        return cost.reshape(-1, 1)

    @staticmethod
    def backward(ctx, dcost):
        dpred, = ctx.saved_tensors
        if isinstance(ctx.loss_scale, torch.Tensor) or ctx.loss_scale != 1.0:
            # the product is formed in fp32 and rounded once: d cost / d y can be ~1 / y, dcost ~1 / batch
            return (dpred.float() * (dcost.reshape(-1, 1, 1).float() * ctx.loss_scale)).to(dpred.dtype), None, None, None, None
        return dpred * dcost.reshape(-1, 1, 1).to(dpred.dtype), None, None, None, None


def ctc_cost_and_grad(y_pred, labels, input_length, label_length):
    """(cost (B,), d cost / d y_pred) of qk_ctc_batch_cost as plain tensors (no autograd node): for callers that chain the gradient
    themselves (layers._DenseSoftmaxCtcMeanFn)."""
    _require_device(y_pred, 'ctc_cost_and_grad')
    return _ctc_call(y_pred.contiguous(), labels, input_length, label_length, True)


def ctc_shape_supported(frames, classes, max_label_len):
    """The shapes qk_ctc_batch_cost takes: C <= 256 classes, at most 127 labels per sample, and one sample's working set
    (T + 8 Lmax + 4 + 2 C + 4 floats) within 64 KB of LDS."""
    return classes <= 256 and max_label_len <= 127 and (frames + 8 * max_label_len + 4 + 2 * classes + 4) * 4 <= 64 * 1024


def ctc_supported(y_pred, labels):
    """qk_ctc_batch_cost takes a contiguous (B, T, C) device tensor of a shape ctc_shape_supported accepts."""
    return (y_pred.is_cuda and y_pred.dtype in _DTYPES and y_pred.dim() == 3 and y_pred.shape[0] > 0 and labels.dim() == 2
            and ctc_shape_supported(y_pred.shape[1], y_pred.shape[2], labels.shape[1]))


def loss_scale_arg(loss_scale, device=None):
    """A loss_scale argument checked without a host read: a positive finite number comes back as a float, a one-element float32
    device tensor (on `device` when given) as it is."""
    if isinstance(loss_scale, torch.Tensor):
        if (loss_scale.dtype != torch.float32 or loss_scale.numel() != 1 or not loss_scale.is_cuda
                or (device is not None and loss_scale.device != device)):
            raise TypeError('a tensor loss_scale must be a one-element float32 tensor on the device of the data')
        return loss_scale.detach()
    if not (loss_scale > 0 and math.isfinite(loss_scale)):
        raise ValueError('loss_scale must be a positive finite number')
    return float(loss_scale)


def ctc_batch_cost(y_pred, labels, input_length, label_length, loss_scale=1.0):
    """K.ctc_batch_cost(labels, y_pred, input_length, label_length) (interspeech_model.py:37-39): per-sample CTC cost (B, 1) of
    the softmax outputs y_pred (B, T, C), blank = C - 1, Keras / TensorFlow semantics (include/qk.h: qk_ctc_batch_cost).

    loss_scale: the GRADIENT this node sends back is multiplied by it (the cost it returns is not) -- static loss scaling for
    float16 activations: under the CTC cost the gradients of the TIMIT body layers sit at 2^-18.5 (profiles/r04_loss_ab.txt), below
    float16's normal range (2^-14); a power of two (2^12 recommended) moves them into it exactly, and the optimiser undoes it in
    fp32: `adam_step(grad_scale=1 / (world * loss_scale))`.  bfloat16 / float32 need none.
    A one-element float32 DEVICE tensor is taken as well (training.GradGuard.loss_scale, the dynamic scale): it is multiplied in on
    the device when the backward runs and never read on the host."""
    _require_device(y_pred, 'ctc_batch_cost')
    return _CtcFn.apply(y_pred.contiguous(), labels, input_length, label_length, loss_scale_arg(loss_scale, y_pred.device))


# ---- transducer (RNN-T) loss (include/qk_rnnt.h) ------------------------------------------------------------------------------------
def rnnt_supported(logits, labels):
    """qk_rnnt_loss takes a contiguous (B, T, Lmax + 1, V) device tensor with labels (B, Lmax), within the limits of
    include/qk_rnnt.h (2 <= V <= 256, Lmax <= 127, T >= 1)."""
    if not (logits.is_cuda and logits.dtype in _DTYPES and logits.dim() == 4 and labels.dim() == 2 and logits.shape[0] > 0
            and labels.shape[0] == logits.shape[0] and labels.shape[1] + 1 == logits.shape[2]):
        return False
    b, t, u1, v = logits.shape
    return bool(L.lib().qk_rnnt_supported(_DTYPES[logits.dtype], b, t, u1, v))


def _rnnt_call(logits, labels, input_length, label_length, want_grad):
    if logits.dim() != 4:
        raise ValueError('rnnt_loss: logits must be (B, T, Lmax + 1, V), got shape %s' % (tuple(logits.shape),))
    b, t, u1, v = logits.shape
    lab = labels.to(device=logits.device, dtype=torch.int32).reshape(b, -1).contiguous()
    if lab.shape[1] + 1 != u1:
        raise ValueError('rnnt_loss: logits have %d label positions, labels (B, %d) need %d' % (u1, lab.shape[1], lab.shape[1] + 1))
    il = input_length.reshape(-1).to(device=logits.device, dtype=torch.int32).contiguous()
    ll = label_length.reshape(-1).to(device=logits.device, dtype=torch.int32).contiguous()
    if il.numel() != b or ll.numel() != b:
        raise ValueError('rnnt_loss: input_length and label_length must have %d elements' % b)
    cost = torch.empty(b, dtype=torch.float32, device=logits.device)
    grad = torch.empty_like(logits) if want_grad else None
    n = int(L.lib().qk_rnnt_workspace_bytes(b, t, u1, v))
    ws = torch.empty(max(n, 16), dtype=torch.uint8, device=logits.device)
    with _on_device(logits.device):
        rc = L.lib().qk_rnnt_loss(_DTYPES[logits.dtype], b, t, u1, v, _ptr(logits), _ptr(lab) if lab.numel() else None, _ptr(il),
                                  _ptr(ll), _ptr(cost), _ptr(grad), _ptr(ws), n, _stream(logits))
    L.check(rc, 'qk_rnnt_loss')
    return cost, grad


class _RnntFn(torch.autograd.Function):
    """qk_rnnt_loss: cost and d cost / d logits from one call; the backward only scales the stored gradient."""

    @staticmethod
    def forward(ctx, logits, labels, input_length, label_length, loss_scale=1.0):
        cost, grad = _rnnt_call(logits, labels, input_length, label_length, ctx.needs_input_grad[0])
        ctx.save_for_backward(grad)
        ctx.loss_scale = loss_scale if isinstance(loss_scale, torch.Tensor) else float(loss_scale)
        return cost.reshape(-1, 1)

    @staticmethod
    def backward(ctx, dcost):
        grad, = ctx.saved_tensors
        if isinstance(ctx.loss_scale, torch.Tensor) or ctx.loss_scale != 1.0:
            # the product is formed in fp32 and rounded once, as in _CtcFn
            return (grad.float() * (dcost.reshape(-1, 1, 1, 1).float() * ctx.loss_scale)).to(grad.dtype), None, None, None, None
        return grad * dcost.reshape(-1, 1, 1, 1).to(grad.dtype), None, None, None, None


def rnnt_cost_and_grad(logits, labels, input_length, label_length):
    """(cost (B,), d cost / d logits) of qk_rnnt_loss as plain tensors (no autograd node)."""
    _require_device(logits, 'rnnt_cost_and_grad')
    return _rnnt_call(logits.contiguous(), labels, input_length, label_length, True)


def rnnt_loss(logits, labels, input_length, label_length, loss_scale=1.0):
    """Transducer (RNN-T) cost per sample, (B, 1) float32, of the joint's UNNORMALISED outputs logits (B, T, Lmax + 1, V), blank =
    V - 1 (include/qk_rnnt.h has the recursion, the fused log-softmax gradient and the conventions for padding cells and
    infeasible rows).  labels (B, Lmax) int; input_length, label_length (B,) or (B, 1).  Three launches; the gradient is stored by
    the forward and the backward only scales it.  loss_scale multiplies the GRADIENT sent back (not the cost), exactly as in
    ctc_batch_cost: a number or a one-element float32 device tensor."""
    _require_device(logits, 'rnnt_loss')
    return _RnntFn.apply(logits.contiguous(), labels, input_length, label_length, loss_scale_arg(loss_scale, logits.device))


# ---- CTC decoding (include/qk.h, "CTC decoding") ----------------------------------------------------------------------------------
CTC_MAX_BEAM, CTC_MAX_CLASSES, EDIT_MAX_REF = 128, 256, 1024


def _length_arg(v, b, device, what, name):
    """A (B,) or (B, 1) length argument, checked (shapes first: a bad shape is refused on any device) but not yet moved."""
    if not torch.is_tensor(v):
        v = torch.as_tensor(v)
    if v.numel() != b or (v.dim() == 2 and v.shape[1] != 1) or v.dim() > 2:
        raise ValueError('%s: %s must have shape (B,) or (B, 1), got %s' % (what, name, tuple(v.shape)))
    if v.is_cuda and v.device != device:
        raise ValueError('%s: %s is on %s, y_pred on %s' % (what, name, v.device, device))
    return v.reshape(-1)


def _decode_args(y_pred, input_length, what):
    _require_device(y_pred, what)
    if y_pred.dim() != 3 or min(y_pred.shape) < 1:
        raise ValueError('%s: y_pred must be a non-empty (B, T, C) tensor, got shape %s' % (what, tuple(y_pred.shape)))
    b, t, c = y_pred.shape
    if c < 2 or c > CTC_MAX_CLASSES:
        raise ValueError('%s: %d classes; the decoders take 2 <= classes <= %d' % (what, c, CTC_MAX_CLASSES))
    il = _length_arg(input_length, b, y_pred.device, what, 'input_length')
    return y_pred.contiguous(), il.to(device=y_pred.device, dtype=torch.int32).contiguous()


def _beam_args(what, beam_width, top_paths):
    beam_width, top_paths = int(beam_width), int(top_paths)
    if not 1 <= beam_width <= CTC_MAX_BEAM:
        raise ValueError('%s: beam_width %d outside 1 .. %d' % (what, beam_width, CTC_MAX_BEAM))
    if not 1 <= top_paths <= beam_width:
        raise ValueError('%s: top_paths %d outside 1 .. beam_width (%d)' % (what, top_paths, beam_width))
    return beam_width, top_paths


def _beam_buffers(y, beam_width, top_paths):
    """(decoded, decoded_len, log_prob, workspace) of a beam search over y (B, T, C)."""
    b, t, _ = y.shape
    dec = torch.empty((top_paths, b, t), dtype=torch.int32, device=y.device)
    dlen = torch.empty((top_paths, b), dtype=torch.int32, device=y.device)
    lp = torch.empty((b, top_paths), dtype=torch.float32, device=y.device)
    ws = torch.empty(int(L.lib().qk_ctc_beam_workspace_bytes(b, t, beam_width)), dtype=torch.uint8, device=y.device)
    return dec, dlen, lp, ws


def ctc_greedy_decode(y_pred, input_length):
    """K.ctc_decode(y_pred, input_length, greedy=True) = tf.nn.ctc_greedy_decoder(merge_repeated=True) as one launch
    (qk_ctc_greedy_decode).  y_pred (B, T, C) softmax outputs (float32 / bfloat16 / float16), blank = C - 1; only the first
    min(max(input_length[b], 0), T) frames count.  Per frame the argmax class (lowest index on ties), runs merged, blanks dropped.

    Returns (decoded (B, T) int32 padded with -1, decoded_len (B,) int32, log_prob (B,) float32) on y_pred's device, without a
    host sync.  log_prob = -sum_t max_c log(y_pred[t][c] + 1e-7): TensorFlow's neg_sum_logits, sign included, which Keras passes
    through under the name log_prob -- mirrored as is."""
    y, il = _decode_args(y_pred, input_length, 'ctc_greedy_decode')
    b, t, c = y.shape
    dec = torch.empty((b, t), dtype=torch.int32, device=y.device)
    dlen = torch.empty(b, dtype=torch.int32, device=y.device)
    lp = torch.empty(b, dtype=torch.float32, device=y.device)
    with _on_device(y.device):
        rc = L.lib().qk_ctc_greedy_decode(_DTYPES[y.dtype], b, t, c, _ptr(y), _ptr(il), _ptr(dec), _ptr(dlen), _ptr(lp), _stream(y))
    L.check(rc, 'qk_ctc_greedy_decode')
    return dec, dlen, lp


def ctc_beam_search_decode(y_pred, input_length, beam_width=100, top_paths=1, merge_repeated=True):
    """K.ctc_decode(y_pred, input_length, greedy=False, beam_width, top_paths) -- a CTC prefix beam search without a language model (ctc_beam_search_decode_lm fuses one),
    one workgroup per sample (qk_ctc_beam_search_decode).  Per frame each beam stays (blank or repeat of its last label) or is
    extended by a non-blank class; an extension equal to an existing beam is merged into it; the beam_width best candidates by total
    log-probability are kept (ties: stay before extension, then lower source rank, then lower class).

    Returns (decoded (top_paths, B, T) int32 padded with -1, decoded_len (top_paths, B) int32, log_prob (B, top_paths) float32),
    paths in descending order of log_prob, without a host sync.  Deviations from TensorFlow: log_prob is the NORMALISED
    log p(prefix | y_pred) (TensorFlow reports scores shifted per frame; the ranking is identical, every candidate consumes one emission
    per frame); paths beyond the number of distinct beams come back empty with log_prob -inf (TensorFlow raises).
    merge_repeated (True, the TF 1.x default Keras 2.x calls) collapses consecutive equal labels of the returned prefix; log_prob stays
    that of the uncollapsed prefix.  Limits: beam_width <= 128, top_paths <= beam_width, C <= 256."""
    beam_width, top_paths = _beam_args('ctc_beam_search_decode', beam_width, top_paths)
    y, il = _decode_args(y_pred, input_length, 'ctc_beam_search_decode')
    b, t, c = y.shape
    dec, dlen, lp, ws = _beam_buffers(y, beam_width, top_paths)
    with _on_device(y.device):
        rc = L.lib().qk_ctc_beam_search_decode(_DTYPES[y.dtype], b, t, c, _ptr(y), _ptr(il), beam_width, top_paths, int(bool(merge_repeated)),
                                               _ptr(dec), _ptr(dlen), _ptr(lp), _ptr(ws), ws.numel(), _stream(y))
    L.check(rc, 'qk_ctc_beam_search_decode')
    return dec, dlen, lp


# ---- CTC forced alignment (include/qk.h, "CTC forced alignment") ---------------------------------------------------------------------
CTC_ALIGN_MAX_LABELS = 127
AlignResult = collections.namedtuple('AlignResult', 'path starts ends score')


def ctc_forced_align(y_pred, labels, input_length, label_length):
    """The best CTC path of a known transcript, one launch (qk_ctc_forced_align): which frames belong to which label.  Arguments as
    for ctc_batch_cost: y_pred (B, T, C) softmax outputs (float32 / bfloat16 / float16), blank = C - 1; labels (B, Lmax) int, Lmax <= 127
    (Lmax = 0 is allowed); input_length, label_length (B,) or (B, 1).  Among the paths through blank, l1, blank, ..., lL, blank that
    the alpha recursion allows, the one that maximises sum_t log_softmax(log(y_pred[t] + 1e-7))[class of the path at t] over the first
    input_length[b] frames; ties: stay before s - 1 before s - 2, the final blank before the last label.

    Returns AlignResult(path (B, T) int32: the class per frame, -1 behind input_length; starts, ends (B, Lmax) int32: first frame of
    label i and one past its last, -1 behind label_length; score (B,) float32: the path's log-probability, <= -cost), device
    tensors, without a host read.  A transcript that does not fit its frames gives score -inf and -1 everywhere."""
    what = 'ctc_forced_align'
    if y_pred.dim() != 3 or min(y_pred.shape) < 1:
        raise ValueError('%s: y_pred must be a non-empty (B, T, C) tensor, got shape %s' % (what, tuple(y_pred.shape)))
    b, t, c = y_pred.shape
    if c < 2 or c > CTC_MAX_CLASSES:
        raise ValueError('%s: %d classes; the alignment takes 2 <= classes <= %d' % (what, c, CTC_MAX_CLASSES))
    if not torch.is_tensor(labels):
        labels = torch.as_tensor(labels)
    if labels.dim() != 2 or labels.shape[0] != b:
        raise ValueError('%s: labels must have shape (B, Lmax) with B = %d, got %s' % (what, b, tuple(labels.shape)))
    if labels.shape[1] > CTC_ALIGN_MAX_LABELS:
        raise ValueError('%s: %d label slots; the alignment takes at most %d' % (what, labels.shape[1], CTC_ALIGN_MAX_LABELS))
    if labels.is_cuda and labels.device != y_pred.device:
        raise ValueError('%s: labels are on %s, y_pred on %s' % (what, labels.device, y_pred.device))
    il = _length_arg(input_length, b, y_pred.device, what, 'input_length')
    ll = _length_arg(label_length, b, y_pred.device, what, 'label_length')
    _require_device(y_pred, what)
    y = y_pred.contiguous()
    il = il.to(device=y.device, dtype=torch.int32).contiguous()
    ll = ll.to(device=y.device, dtype=torch.int32).contiguous()
    lab = labels.to(device=y.device, dtype=torch.int32).contiguous()
    lmax = lab.shape[1]
    path = torch.empty((b, t), dtype=torch.int32, device=y.device)
    starts = torch.empty((b, lmax), dtype=torch.int32, device=y.device)
    ends = torch.empty((b, lmax), dtype=torch.int32, device=y.device)
    score = torch.empty(b, dtype=torch.float32, device=y.device)
    n = int(L.lib().qk_ctc_align_workspace_bytes(b, t, lmax))
    ws = torch.empty(n, dtype=torch.uint8, device=y.device)
    nz = lmax > 0
    with _on_device(y.device):
        rc = L.lib().qk_ctc_forced_align(_DTYPES[y.dtype], b, t, c, _ptr(y), _ptr(lab) if nz else None, lmax, _ptr(il), _ptr(ll), _ptr(path),
                                         _ptr(starts) if nz else None, _ptr(ends) if nz else None, _ptr(score), _ptr(ws), n, _stream(y))
    L.check(rc, 'qk_ctc_forced_align')
    return AlignResult(path, starts, ends, score)


CTC_LM_MAX_TRIGRAM_CLASSES = 64


def ctc_beam_search_decode_lm(y_pred, input_length, lm, beam_width=100, top_paths=1, merge_repeated=True, lm_weight=0.5,
                              insertion_bonus=0.0, eos=True):
    """CTC prefix beam search fused with a phone n-gram LM, one workgroup per sample (qk_ctc_beam_search_decode_lm).  Every candidate
    prefix l is ranked by S(l) = log p(l | y_pred) + lm_weight log P_LM(l) + insertion_bonus |l| in place of the total alone (pb / pnb
    recursions, merging and the tie rule as in ctc_beam_search_decode); eos=True re-ranks the final beams by S + lm_weight
    log P(</s> | l).  lm: a qcnn_amd.lm.NgramLM over C - 1 labels (order 1 to 3; order 3 for C <= 64).  lm_weight must be finite
    and >= 0, insertion_bonus finite; lm_weight = insertion_bonus = 0 returns ctc_beam_search_decode's results bit for bit.

    Returns (decoded (top_paths, B, T) int32 padded with -1, decoded_len (top_paths, B) int32, log_prob (B, top_paths) float32 = the
    acoustic log p(prefix | y_pred), score (B, top_paths) float32 = the S the paths were ranked by), without a host sync; empty paths
    have -inf in both.  merge_repeated collapses the output; the LM scored the uncollapsed prefix."""
    what = 'ctc_beam_search_decode_lm'
    beam_width, top_paths = _beam_args(what, beam_width, top_paths)
    lm_weight, insertion_bonus = float(lm_weight), float(insertion_bonus)
    if not (math.isfinite(lm_weight) and lm_weight >= 0.0):
        raise ValueError('%s: lm_weight must be finite and >= 0, got %r' % (what, lm_weight))
    if not math.isfinite(insertion_bonus):
        raise ValueError('%s: insertion_bonus must be finite, got %r' % (what, insertion_bonus))
    order = int(lm.order)
    if not 1 <= order <= 3:
        raise ValueError('%s: LM order %d outside 1 .. 3' % (what, order))
    if torch.is_tensor(y_pred) and y_pred.dim() == 3:          # LM / shape checks first: they need no device
        c = y_pred.shape[2]
        if lm.num_labels != c - 1:
            raise ValueError('%s: the LM has %d labels, y_pred %d classes (%d labels + blank)' % (what, lm.num_labels, c, c - 1))
        if order == 3 and c > CTC_LM_MAX_TRIGRAM_CLASSES:
            raise ValueError('%s: a trigram LM needs C <= %d, got %d' % (what, CTC_LM_MAX_TRIGRAM_CLASSES, c))
    y, il = _decode_args(y_pred, input_length, what)
    b, t, c = y.shape
    table = lm.table(y.device)
    if tuple(table.shape) != (c ** (order - 1), c) or table.dtype != torch.float32:
        raise ValueError('%s: LM table of shape %s %s, expected (%d, %d) float32' % (what, tuple(table.shape), table.dtype,
                                                                                     c ** (order - 1), c))
    dec, dlen, lp, ws = _beam_buffers(y, beam_width, top_paths)
    score = torch.empty_like(lp)
    with _on_device(y.device):
        rc = L.lib().qk_ctc_beam_search_decode_lm(_DTYPES[y.dtype], b, t, c, _ptr(y), _ptr(il), beam_width, top_paths,
                                                  int(bool(merge_repeated)), order, _ptr(table), lm_weight, insertion_bonus,
                                                  int(bool(eos)), _ptr(dec), _ptr(dlen), _ptr(lp), _ptr(score), _ptr(ws), ws.numel(), _stream(y))
    L.check(rc, 'qk_ctc_beam_search_decode_lm')
    return dec, dlen, lp, score


def _token_args(seq, length, what, name):
    if not torch.is_tensor(seq) or not seq.is_cuda:
        raise RuntimeError('%s: got a CPU tensor for %s. Decoding runs only on the MI355X HIP path (libqk_hip.so); there is no CPU '
                           'fallback.' % (what, name))
    if seq.dim() != 2:
        raise ValueError('%s: %s must be a (B, L) tensor, got shape %s' % (what, name, tuple(seq.shape)))
    b = seq.shape[0]
    ln = length if torch.is_tensor(length) else torch.as_tensor(length)
    if ln.numel() != b:
        raise ValueError('%s: %s length must have B = %d entries, got %d' % (what, name, b, ln.numel()))
    return (seq.to(dtype=torch.int32).contiguous(),
            ln.reshape(-1).to(device=seq.device, dtype=torch.int32).contiguous())


def _pair_args(what, hyp, hyp_len, ref, ref_len, class_map, between=None):
    """(hyp, hyp_len, ref, ref_len, class_map or None, classes) of a scoring call as int32 device tensors: the two token arguments,
    their devices, then between(hyp, ref) -- the caller's own checks, which come before the class map's -- then the class map."""
    h, hl = _token_args(hyp, hyp_len, what, 'hyp')
    r, rl = _token_args(ref, ref_len, what, 'ref')
    if h.device != r.device:
        raise ValueError('%s: hyp on %s, ref on %s' % (what, h.device, r.device))
    if between is not None:
        between(h, r)
    cm, classes = None, 0
    if class_map is not None:
        cm = torch.as_tensor(class_map).reshape(-1).to(device=h.device, dtype=torch.int32).contiguous()
        classes = cm.numel()
        if classes < 1:
            raise ValueError('%s: empty class_map' % what)
    return h, hl, r, rl, cm, classes


def _edit_distance(hyp, hyp_len, ref, ref_len, class_map=None):
    what = 'edit_distance'

    def shapes(h, r):
        if h.shape[0] != r.shape[0]:
            raise ValueError('%s: %d hypotheses, %d references' % (what, h.shape[0], r.shape[0]))
        if r.shape[1] > EDIT_MAX_REF:
            raise ValueError('%s: references of up to %d tokens are supported, got %d' % (what, EDIT_MAX_REF, r.shape[1]))

    h, hl, r, rl, cm, classes = _pair_args(what, hyp, hyp_len, ref, ref_len, class_map, shapes)
    b = h.shape[0]
    dist = torch.empty(b, dtype=torch.int32, device=h.device)
    rlen = torch.empty(b, dtype=torch.int32, device=h.device)
    if b == 0:
        return dist, rlen
    with _on_device(h.device):
        rc = L.lib().qk_edit_distance(b, _ptr(h), h.shape[1], _ptr(hl), _ptr(r), r.shape[1], _ptr(rl), _ptr(cm), classes, _ptr(dist),
                                      _ptr(rlen), _stream(h))
    L.check(rc, 'qk_edit_distance')
    return dist, rlen


def edit_distance(hyp, hyp_len, ref, ref_len, class_map=None):
    """tf.edit_distance(normalize=False) per pair as one launch (qk_edit_distance): Levenshtein distance with unit costs between
    hyp[b, :hyp_len[b]] and ref[b, :ref_len[b]] (device int tensors (B, Lh) / (B, Lr), Lr <= 1024, any Lh).  class_map (C,) int: a
    token t in [0, C) becomes class_map[t] in both sequences and is dropped when that is -1 (e.g. the TIMIT 61 -> 39 folding).
    Returns (B,) int32 on the device, without a host sync."""
    return _edit_distance(hyp, hyp_len, ref, ref_len, class_map)[0]


# ---- Scoring alignment (include/qk.h, "Scoring alignment") ---------------------------------------------------------------------------
EDIT_ALIGN_MAX_SEQ = 1024
EDIT_ALIGN_MAX_CLASSES = 256
EditAlignment = collections.namedtuple('EditAlignment', 'ref hyp length counts')


def edit_alignment(hyp, hyp_len, ref, ref_len, class_map=None, confusion=None, align=True):
    """The Levenshtein alignment behind edit_distance, one launch (qk_edit_align): hyp (B, Lh), ref (B, Lr) device int tensors with
    Lh, Lr <= 1024, hyp_len / ref_len (B,), class_map as in edit_distance.  Read backwards from the end, the alignment takes the
    diagonal (correct or substitution) when it is optimal, otherwise a deletion when that is optimal, otherwise an insertion.

    Returns EditAlignment(ref, hyp (B, Lh + Lr) int32: the aligned pairs in forward order as mapped tokens, hyp = -1 a deletion,
    ref = -1 an insertion, both -1 behind length; length (B,) int32; counts (B, 4) int32: correct, substitutions, deletions,
    insertions), device tensors, without a host read.  align=False is the counts-only call: ref, hyp and length are None.
    confusion: a caller-owned (K + 1, K + 1) int32 contiguous tensor on the same device, ACCUMULATED in place: [r][h] += 1 per
    aligned pair, row K the insertions, column K the deletions; pairs with a token outside [0, K) are counted but left out of it."""
    what = 'edit_alignment'
    # shapes first (a bad shape is refused on any device), then the device
    if torch.is_tensor(hyp) and torch.is_tensor(ref) and hyp.dim() == 2 and ref.dim() == 2:
        if hyp.shape[0] != ref.shape[0]:
            raise ValueError('%s: %d hypotheses, %d references' % (what, hyp.shape[0], ref.shape[0]))
        if max(hyp.shape[1], ref.shape[1]) > EDIT_ALIGN_MAX_SEQ:
            raise ValueError('%s: sequences of up to %d tokens are supported, got hyp %d, ref %d' % (what, EDIT_ALIGN_MAX_SEQ, hyp.shape[1],
                                                                                                     ref.shape[1]))
    k = 0
    if confusion is not None:
        if (not torch.is_tensor(confusion) or confusion.dim() != 2 or confusion.shape[0] != confusion.shape[1] or confusion.shape[0] < 1
                or confusion.dtype != torch.int32 or not confusion.is_contiguous()):
            raise ValueError('%s: confusion must be a square (K + 1, K + 1) int32 contiguous tensor' % what)
        k = confusion.shape[0] - 1
        if k > EDIT_ALIGN_MAX_CLASSES:
            raise ValueError('%s: a confusion matrix of up to %d classes is supported, got %d' % (what, EDIT_ALIGN_MAX_CLASSES, k))
    def confusion_device(h, r):
        if confusion is not None and confusion.device != h.device:
            raise ValueError('%s: confusion on %s, hyp on %s' % (what, confusion.device, h.device))

    h, hl, r, rl, cm, classes = _pair_args(what, hyp, hyp_len, ref, ref_len, class_map, confusion_device)
    b, a = h.shape[0], h.shape[1] + r.shape[1]
    counts = torch.empty((b, 4), dtype=torch.int32, device=h.device)
    ali_ref = ali_hyp = ali_len = None
    if align:
        ali_ref = torch.empty((b, a), dtype=torch.int32, device=h.device)
        ali_hyp = torch.empty((b, a), dtype=torch.int32, device=h.device)
        ali_len = torch.empty(b, dtype=torch.int32, device=h.device)
    if b == 0:
        return EditAlignment(ali_ref, ali_hyp, ali_len, counts)
    n = int(L.lib().qk_edit_align_workspace_bytes(b, h.shape[1], r.shape[1]))
    ws = torch.empty(n, dtype=torch.uint8, device=h.device) if n else None
    with _on_device(h.device):
        rc = L.lib().qk_edit_align(b, _ptr(h), h.shape[1], _ptr(hl), _ptr(r), r.shape[1], _ptr(rl), _ptr(cm), classes, _ptr(counts),
                                   _ptr(ali_ref), _ptr(ali_hyp), _ptr(ali_len), _ptr(confusion), k, _ptr(ws), n, _stream(h))
    L.check(rc, 'qk_edit_align')
    return EditAlignment(ali_ref, ali_hyp, ali_len, counts)


# ---- Acoustic front end (include/qk.h, "Acoustic front end") -------------------------------------------------------------------
def fbank_quaternion(wave, lengths, frames, frame_len, frame_step, nfft, preemph, window, mel_bins, append_energy, delta_n, normalize,
                     dtype):
    """Waveforms -> (B, 4, F, frames) quaternion filter-bank features as one call of qk_fbank_quaternion (two launches, three when
    normalising).  wave (B, n_max) int16 / float32 on the device, lengths (B,) int32 samples per utterance (same device); mel_bins a
    host sequence of nfilt + 2 FFT bin edges; window / normalize are the QK_WINDOW_* / QK_FBANK_NORM_* codes.  Returns
    (features in `dtype`, frame_lengths (B,) int32) without a host sync.  The user-facing entry point, with the recipe's parameters
    in seconds and hertz, is qcnn_amd.features.quaternion_fbank."""
    if not torch.is_tensor(wave) or not wave.is_cuda:
        raise RuntimeError('fbank_quaternion: got a CPU tensor. The acoustic front end runs only on the MI355X HIP path (libqk_hip.so); '
                           'there is no CPU fallback.')
    if wave.dtype not in (torch.int16, torch.float32):
        raise TypeError('fbank_quaternion: waveforms must be int16 or float32, got %s' % wave.dtype)
    if dtype not in _DTYPES:
        raise TypeError('fbank_quaternion: unsupported output dtype %s (float32, bfloat16, float16)' % dtype)
    if wave.dim() != 2 or min(wave.shape) < 1:
        raise ValueError('fbank_quaternion: wave must be a non-empty (B, samples) tensor, got shape %s' % (tuple(wave.shape),))
    if lengths.device != wave.device or lengths.dtype != torch.int32 or lengths.shape != (wave.shape[0],):
        raise ValueError('fbank_quaternion: lengths must be a (B,) int32 tensor on %s' % wave.device)
    wave, lengths = wave.contiguous(), lengths.contiguous()
    b, n_max = wave.shape
    nfilt = len(mel_bins) - 2
    rows = nfilt + (1 if append_energy else 0)
    out = torch.empty((b, 4, rows, frames), dtype=dtype, device=wave.device)
    flen = torch.empty(b, dtype=torch.int32, device=wave.device)
    n = int(L.lib().qk_fbank_workspace_bytes(b, frames, rows, int(normalize)))
    ws = torch.empty(n, dtype=torch.uint8, device=wave.device)
    bins = (ctypes.c_int32 * len(mel_bins))(*[int(v) for v in mel_bins])
    wd = L.QK_WAVE_I16 if wave.dtype == torch.int16 else L.QK_WAVE_F32
    with _on_device(wave.device):
        rc = L.lib().qk_fbank_quaternion(wd, b, n_max, _ptr(wave), _ptr(lengths), frames, frame_len, frame_step, nfft, float(preemph),
                                         int(window), nfilt, bins, int(bool(append_energy)), int(delta_n), int(normalize), _DTYPES[dtype],
                                         _ptr(out), _ptr(flen), _ptr(ws), n, _stream(wave))
    L.check(rc, 'qk_fbank_quaternion')
    return out, flen


# ---- SpecAugment (include/qk.h, "SpecAugment") ----------------------------------------------------------------------------------
def _specaug_policy(what, time_warp, freq_masks, freq_width, time_masks, time_width, time_ratio, fill, seed):
    """The checked qk_specaug_t of a policy; ValueError / TypeError on the host, before any device is touched."""
    vals = {}
    for name, v in (('time_warp', time_warp), ('freq_masks', freq_masks), ('freq_width', freq_width), ('time_masks', time_masks),
                    ('time_width', time_width), ('seed', seed)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise TypeError('%s: %s must be an integer, got %r' % (what, name, v))
        vals[name] = v
    for name in ('freq_masks', 'time_masks'):
        if not 0 <= vals[name] <= L.QK_SPECAUG_MAX_MASKS:
            raise ValueError('%s: %s %d outside 0 .. %d' % (what, name, vals[name], L.QK_SPECAUG_MAX_MASKS))
    for name in ('time_warp', 'freq_width', 'time_width'):
        if not 0 <= vals[name] < 2 ** 30:
            raise ValueError('%s: %s must be >= 0 (and < 2^30), got %d' % (what, name, vals[name]))
    if not 0 <= vals['seed'] <= 0xFFFFFFFF:
        raise ValueError('%s: seed must fit 32 unsigned bits, got %d' % (what, vals['seed']))
    for name, v in (('time_ratio', time_ratio), ('fill', fill)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError('%s: %s must be a finite number, got %r' % (what, name, v))
    if not 0.0 <= time_ratio <= 1.0:
        raise ValueError('%s: time_ratio %r outside [0, 1]' % (what, time_ratio))
    return L.SpecAugPolicy(vals['time_warp'], vals['freq_masks'], vals['freq_width'], vals['time_masks'], vals['time_width'],
                           float(time_ratio), float(fill), vals['seed'])


def spec_augment(x, lengths, *, time_warp=0, freq_masks=0, freq_width=0, time_masks=0, time_width=0, time_ratio=1.0, fill=0.0, seed=0,
                 counter=None, dtype=None, return_plan=False):
    """SpecAugment of the model's channels_first input as one launch (qk_spec_augment; semantics: include/qk.h, "SpecAugment").

    x (B, planes, rows, T) float32 / bfloat16 / float16 on the device; lengths (B,) valid frames per utterance (clamped to [0, T]).
    Per utterance: a time warp that moves one frame by up to time_warp frames (linear interpolation, fp32), freq_masks masks of up
    to freq_width rows, time_masks masks of up to min(time_width, time_ratio n) frames, written as `fill`.  Every plane of an
    utterance gets the same warp and masks (a cell is one quaternion); the derivative planes are NOT rescaled by the warp's slope.
    Frames >= lengths[b] are copied.  The draws are a hash of (seed, counter, utterance): equal arguments give equal bits.
    counter: one-element int32 / uint32 DEVICE tensor read by the kernel (None: 0) -- advance it with a device op and a captured
    graph draws new masks on every replay.  dtype: output dtype (default x.dtype).  Returns a new tensor (never x itself), or
    (out, plan) with return_plan: plan (B, 36) int32 on the device = {n, c, w, 0, (f0, fw) x 8, (t0, tw) x 8}.  No host sync."""
    what = 'spec_augment'
    pol = _specaug_policy(what, time_warp, freq_masks, freq_width, time_masks, time_width, time_ratio, fill, seed)
    if dtype is None and torch.is_tensor(x):
        dtype = x.dtype
    if dtype not in _DTYPES:
        raise TypeError('%s: unsupported output dtype %s (float32, bfloat16, float16)' % (what, dtype))
    if not torch.is_tensor(x) or not x.is_cuda:
        raise RuntimeError('%s: got a CPU tensor. SpecAugment runs only on the MI355X HIP path (libqk_hip.so); there is no CPU '
                           'fallback.' % what)
    if x.dtype not in _DTYPES:
        raise TypeError('%s: unsupported input dtype %s (float32, bfloat16, float16)' % (what, x.dtype))
    if x.dim() != 4 or min(x.shape) < 1:
        raise ValueError('%s: x must be a non-empty (B, planes, rows, T) tensor, got shape %s' % (what, tuple(x.shape)))
    b, planes, rows, frames = x.shape
    lengths = lengths if torch.is_tensor(lengths) else torch.as_tensor(lengths)
    if lengths.numel() != b:
        raise ValueError('%s: lengths must have B = %d entries, got %d' % (what, b, lengths.numel()))
    lengths = lengths.reshape(-1).to(device=x.device, dtype=torch.int32).contiguous()
    if counter is not None:
        if (not torch.is_tensor(counter) or counter.device != x.device or counter.numel() != 1
                or counter.dtype not in (torch.int32, torch.uint32)):
            raise ValueError('%s: counter must be a one-element int32 / uint32 tensor on %s' % (what, x.device))
    x = x.contiguous()
    out = torch.empty(x.shape, dtype=dtype, device=x.device)
    plan = torch.empty((b, L.QK_SPECAUG_PLAN_WORDS), dtype=torch.int32, device=x.device) if return_plan else None
    with _on_device(x.device):
        rc = L.lib().qk_spec_augment(_DTYPES[x.dtype], _DTYPES[dtype], b, planes, rows, frames, _ptr(x), _ptr(lengths), ctypes.byref(pol),
                                     _ptr(counter), _ptr(out), _ptr(plan), _stream(x))
    L.check(rc, 'qk_spec_augment')
    return (out, plan) if return_plan else out


# ---- Speed and volume perturbation (include/qk.h, "Speed and volume perturbation") ---------------------------------------------
DEFAULT_SPEEDS = ((9, 10), (1, 1), (11, 10))
_speed_tables_host = {}         # (speeds, zeros, rolloff) -> speed_perturb_tables' dict
_speed_tables_dev = {}          # (speeds, zeros, rolloff, device) -> the float32 tables on that device


def _speed_args(what, speeds, gain, zeros, rolloff, seed):
    """The checked (speeds as a tuple of int pairs, (gain_lo, gain_hi)); ValueError / TypeError on the host, before any device is
    touched."""
    try:
        speeds = tuple(tuple(s) for s in speeds)
    except TypeError:
        raise TypeError('%s: speeds must be a sequence of (num, den) pairs, got %r' % (what, speeds))
    if not 1 <= len(speeds) <= L.QK_SPEED_MAX_SPEEDS:
        raise ValueError('%s: between 1 and %d speeds, got %d' % (what, L.QK_SPEED_MAX_SPEEDS, len(speeds)))
    for s in speeds:
        if len(s) != 2:
            raise ValueError('%s: a speed is a (num, den) pair, got %r' % (what, s))
        for v in s:
            if isinstance(v, bool) or not isinstance(v, int):
                raise TypeError('%s: a speed is a pair of integers, got %r (write 0.9 as (9, 10))' % (what, s))
        num, den = s
        if not (1 <= num <= L.QK_SPEED_MAX_DEN and 1 <= den <= L.QK_SPEED_MAX_DEN and den <= 2 * num and num <= 2 * den):
            raise ValueError('%s: speed %d / %d: both must lie in 1 .. %d and the ratio in [1/2, 2]' % (what, num, den, L.QK_SPEED_MAX_DEN))
    try:
        lo, hi = gain
    except (TypeError, ValueError):
        raise ValueError('%s: gain must be a (low, high) pair, got %r' % (what, gain))
    for v in (lo, hi):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError('%s: the gains must be finite numbers, got %r' % (what, gain))
    if not 0.0 <= lo <= hi or hi > 3e38:
        raise ValueError('%s: need 0 <= gain low <= gain high (float32), got %r' % (what, gain))
    if isinstance(zeros, bool) or not isinstance(zeros, int):
        raise TypeError('%s: zeros must be an integer, got %r' % (what, zeros))
    if zeros < 1:
        raise ValueError('%s: zeros must be >= 1, got %d' % (what, zeros))
    if isinstance(rolloff, bool) or not isinstance(rolloff, (int, float)) or not math.isfinite(rolloff) or not 0.0 < rolloff <= 1.0:
        raise ValueError('%s: rolloff must lie in (0, 1], got %r' % (what, rolloff))
    if isinstance(seed, bool) or not isinstance(seed, int):
        raise TypeError('%s: seed must be an integer, got %r' % (what, seed))
    if not 0 <= seed <= 0xFFFFFFFF:
        raise ValueError('%s: seed must fit 32 unsigned bits, got %d' % (what, seed))
    return speeds, (float(lo), float(hi))


def speed_perturb_tables(speeds=DEFAULT_SPEEDS, zeros=6, rolloff=0.99):
    """The polyphase filter tables of a set of speeds, built on the host (include/qk.h, "Filter table": torchaudio's
    sinc_interp_hann, float64, rounded once to float32), and the policy fields that go with them.  Returns a dict: num, den,
    half_width, table_offset (lists, one entry per speed; half_width 0 and no table where num == den) and tables, one float32
    NumPy array that holds speed i's (den, 2 half_width + 2) matrix from table_offset[i] on.  Cached per (speeds, zeros, rolloff);
    speed_perturb keeps one device copy per device."""
    speeds, _ = _speed_args('speed_perturb_tables', speeds, (1.0, 1.0), zeros, rolloff, 0)
    key = (speeds, zeros, float(rolloff))
    hit = _speed_tables_host.get(key)
    if hit is not None:
        return hit
    half_width, offsets, parts, at = [], [], [], 0
    for p, q in speeds:
        if p == q:
            half_width.append(0)
            offsets.append(0)
            continue
        fc = float(rolloff) * min(1.0, q / p)
        kw = int(math.ceil(zeros / fc))
        if 2 * kw + 2 > L.QK_SPEED_MAX_TAPS:
            raise ValueError('speed_perturb_tables: speed %d / %d with zeros %d and rolloff %r needs %d taps, more than %d'
                             % (p, q, zeros, rolloff, 2 * kw + 2, L.QK_SPEED_MAX_TAPS))
        r = np.arange(q, dtype=np.float64)[:, None]
        j = np.arange(-kw, kw + 2, dtype=np.float64)[None, :]
        t = fc * (r / q - j)
        tab = np.where(np.abs(t) < zeros, fc * np.sinc(t) * np.cos(np.pi * t / (2.0 * zeros)) ** 2, 0.0)
        half_width.append(kw)
        offsets.append(at)
        parts.append(tab.astype(np.float32).reshape(-1))
        at += tab.size
    tables = np.concatenate(parts) if parts else np.zeros(0, dtype=np.float32)
    tables.setflags(write=False)
    hit = dict(num=[s[0] for s in speeds], den=[s[1] for s in speeds], half_width=half_width, table_offset=offsets, tables=tables)
    _speed_tables_host[key] = hit
    return hit


def _speed_policy(speeds, gain, zeros, rolloff, seed):
    """(qk_speed_perturb_t, host tables dict, cache key) of checked arguments."""
    tab = speed_perturb_tables(speeds, zeros, rolloff)
    pol = L.SpeedPerturbPolicy()
    pol.n_speeds = len(speeds)
    for i in range(len(speeds)):
        pol.num[i], pol.den[i], pol.half_width[i], pol.table_offset[i] = tab['num'][i], tab['den'][i], tab['half_width'][i], tab['table_offset'][i]
    pol.gain_lo, pol.gain_hi, pol.seed = gain[0], gain[1], seed
    return pol, tab, (speeds, zeros, float(rolloff))


def speed_perturb(wave, lengths, *, speeds=DEFAULT_SPEEDS, gain=(1.0, 1.0), zeros=6, rolloff=0.99, seed=0, counter=None,
                  return_plan=False):
    """Speed and volume perturbation of a batch of waveforms as one launch (qk_speed_perturb; semantics: include/qk.h, "Speed and
    volume perturbation").

    wave (B, n_max) int16 / float32 on the device; lengths (B,) valid samples per utterance (clamped to [0, n_max]).  Per utterance
    one of `speeds` ((num, den) pairs: 0.9 is (9, 10)) is drawn and the utterance resampled by it with a windowed-sinc filter of
    `zeros` zero crossings (tempo and pitch change together, as `sox speed` does; speed 11/10 leaves ceil(10 n / 11) samples), and a
    linear gain is drawn from [gain[0], gain[1]).  The draws are a hash of (seed, counter, utterance): equal arguments give equal
    bits.  counter: one-element int32 / uint32 DEVICE tensor read by the kernel (None: 0).

    Returns (out, out_lengths): out (B, ceil(n_max / slowest speed)) float32 at the input's scale, zero from out_lengths[b] on;
    out_lengths (B,) int32 on the device.  With return_plan also plan (B, 4) int32 = {n, speed index, n', bits of the gain}.  No
    host sync; the filter tables are built on the host once per (speeds, zeros, rolloff) and copied once per device."""
    what = 'speed_perturb'
    speeds, gain = _speed_args(what, speeds, gain, zeros, rolloff, seed)
    pol, tab, key = _speed_policy(speeds, gain, zeros, rolloff, seed)
    if torch.is_tensor(wave) and wave.dtype not in (torch.int16, torch.float32):
        raise TypeError('%s: waveforms must be int16 or float32, got %s' % (what, wave.dtype))
    if not torch.is_tensor(wave) or not wave.is_cuda:
        raise RuntimeError('%s: got a CPU tensor. Speed perturbation runs only on the MI355X HIP path (libqk_hip.so); there is no CPU '
                           'fallback.' % what)
    if wave.dim() != 2 or min(wave.shape) < 1:
        raise ValueError('%s: wave must be a non-empty (B, samples) tensor, got shape %s' % (what, tuple(wave.shape)))
    b, n_max = wave.shape
    lengths = lengths if torch.is_tensor(lengths) else torch.as_tensor(lengths)
    if lengths.numel() != b:
        raise ValueError('%s: lengths must have B = %d entries, got %d' % (what, b, lengths.numel()))
    lengths = lengths.reshape(-1).to(device=wave.device, dtype=torch.int32).contiguous()
    if counter is not None:
        if (not torch.is_tensor(counter) or counter.device != wave.device or counter.numel() != 1
                or counter.dtype not in (torch.int32, torch.uint32)):
            raise ValueError('%s: counter must be a one-element int32 / uint32 tensor on %s' % (what, wave.device))
    n_out = int(L.lib().qk_speed_perturb_out_samples(n_max, ctypes.byref(pol)))
    if n_out < 1 or max(n_max, n_out) >= 1 << 26:
        raise ValueError('%s: rows of %d samples (%d after the slowest speed) are not supported (limit 2^26)' % (what, n_max, n_out))
    tables = None
    if tab['tables'].size:
        tables = _speed_tables_dev.get(key + (wave.device,))
        if tables is None:
            tables = torch.from_numpy(tab['tables'].copy()).to(wave.device)
            _speed_tables_dev[key + (wave.device,)] = tables
    wave = wave.contiguous()
    out = torch.empty((b, n_out), dtype=torch.float32, device=wave.device)
    out_lengths = torch.empty(b, dtype=torch.int32, device=wave.device)
    plan = torch.empty((b, L.QK_SPEED_PLAN_WORDS), dtype=torch.int32, device=wave.device) if return_plan else None
    wd = L.QK_WAVE_I16 if wave.dtype == torch.int16 else L.QK_WAVE_F32
    with _on_device(wave.device):
        rc = L.lib().qk_speed_perturb(wd, b, n_max, _ptr(wave), _ptr(lengths), ctypes.byref(pol), _ptr(tables), _ptr(counter), n_out,
                                      _ptr(out), _ptr(out_lengths), _ptr(plan), _stream(wave))
    L.check(rc, 'qk_speed_perturb')
    return (out, out_lengths, plan) if return_plan else (out, out_lengths)


# ---- Reverberation and additive noise (include/qk.h, "Reverberation and additive noise") ----------------------------------------
def _bank_rows(what, name, rows, kinds):
    """The rows of a bank as 1-D NumPy arrays, checked: a non-empty sequence of non-empty 1-D arrays of finite numbers."""
    if isinstance(rows, (str, bytes)) or torch.is_tensor(rows) or isinstance(rows, np.ndarray):
        raise TypeError('%s: %s must be a list of 1-D arrays, got %s' % (what, name, type(rows).__name__))
    try:
        rows = [np.asarray(r) for r in rows]
    except TypeError:
        raise TypeError('%s: %s must be a list of 1-D arrays, got %r' % (what, name, rows))
    if not rows:
        raise ValueError('%s: %s is empty' % (what, name))
    for i, r in enumerate(rows):
        if r.dtype.kind not in kinds:
            raise TypeError('%s: %s[%d] has dtype %s' % (what, name, i, r.dtype))
        if r.ndim != 1 or r.size < 1:
            raise ValueError('%s: %s[%d] must be a non-empty 1-D array, got shape %s' % (what, name, i, r.shape))
        if not np.all(np.isfinite(r)):
            raise ValueError('%s: %s[%d] holds a value that is not finite' % (what, name, i))
    return rows


def prepare_rirs(rirs, max_taps=L.QK_REVERB_MAX_TAPS, device=None):
    """A bank of room impulse responses for noise_reverb / features.NoiseReverb, built on the host in float64: every response (a 1-D
    float array) is cut behind max_taps samples, its direct path is taken as the first argmax of |h| (the output of the
    convolution is shifted by it, so the labels keep their places), it is scaled to unit energy and rounded once to float32; the
    rows are padded with zeros to the longest.  Returns (rirs (R, stride) float32, rir_len (R,) int32, rir_delay (R,) int32) on
    `device` (None: the host) -- what include/qk.h asks of the caller holds by construction."""
    what = 'prepare_rirs'
    if isinstance(max_taps, bool) or not isinstance(max_taps, int):
        raise TypeError('%s: max_taps must be an integer, got %r' % (what, max_taps))
    if not 1 <= max_taps <= L.QK_REVERB_MAX_TAPS:
        raise ValueError('%s: max_taps %d outside 1 .. %d' % (what, max_taps, L.QK_REVERB_MAX_TAPS))
    rows = [r.astype(np.float64)[:max_taps] for r in _bank_rows(what, 'rirs', rirs, 'f')]
    bank = np.zeros((len(rows), max(r.size for r in rows)), dtype=np.float32)
    delay = np.zeros(len(rows), dtype=np.int32)
    for i, h in enumerate(rows):
        energy = float(np.sum(h * h))
        if not energy > 0.0:
            raise ValueError('%s: rirs[%d] is all zeros in its first %d samples' % (what, i, max_taps))
        delay[i] = int(np.argmax(np.abs(h)))
        bank[i, :h.size] = (h / math.sqrt(energy)).astype(np.float32)
    length = np.array([r.size for r in rows], dtype=np.int32)
    return tuple(torch.from_numpy(a).to(device) if device is not None else torch.from_numpy(a) for a in (bank, length, delay))


def prepare_noises(noises, device=None):
    """A bank of noise recordings for noise_reverb / features.NoiseReverb: 1-D int16 or float arrays of any lengths, as float32
    at their own scale (only the ratio of a recording's energy to the utterance's matters), rows padded with zeros to the
    longest.  Returns (noises (N, stride) float32, noise_len (N,) int32) on `device` (None: the host)."""
    rows = _bank_rows('prepare_noises', 'noises', noises, 'fi')
    bank = np.zeros((len(rows), max(r.size for r in rows)), dtype=np.float32)
    for i, v in enumerate(rows):
        bank[i, :v.size] = v.astype(np.float32)
    length = np.array([r.size for r in rows], dtype=np.int32)
    return tuple(torch.from_numpy(a).to(device) if device is not None else torch.from_numpy(a) for a in (bank, length))


def _bank_ok(what, name, bank, parts, max_stride):
    """None, or the bank as a tuple of `parts` tensors: (rows, stride) float32 and (rows,) int32 vectors, all on one device."""
    if bank is None:
        return None
    if not isinstance(bank, (tuple, list)) or len(bank) != parts or not all(torch.is_tensor(t) for t in bank):
        raise TypeError('%s: %s must be None or the %d tensors of prepare_%s, got %r' % (what, name, parts, name, type(bank).__name__))
    rows = bank[0]
    if rows.dtype != torch.float32 or any(t.dtype != torch.int32 for t in bank[1:]):
        raise TypeError('%s: %s must be a float32 matrix and int32 vectors (prepare_%s)' % (what, name, name))
    if rows.dim() != 2 or min(rows.shape) < 1 or any(tuple(t.shape) != (rows.shape[0],) for t in bank[1:]):
        raise ValueError('%s: %s must be a non-empty (rows, stride) matrix with one length per row' % (what, name))
    if max_stride is not None and rows.shape[1] > max_stride:
        raise ValueError('%s: %s rows of %d taps, more than %d' % (what, name, rows.shape[1], max_stride))
    if any(t.device != rows.device for t in bank[1:]):
        raise ValueError('%s: the tensors of %s live on different devices' % (what, name))
    return tuple(bank)


def _env_args(what, rirs, noises, rir_prob, noise_prob, snr, seed):
    """The checked (rirs, noises, qk_noise_reverb_t); ValueError / TypeError on the host, before any device is touched."""
    rirs = _bank_ok(what, 'rirs', rirs, 3, L.QK_REVERB_MAX_TAPS)
    noises = _bank_ok(what, 'noises', noises, 2, None)
    q24 = []
    for name, v in (('rir_prob', rir_prob), ('noise_prob', noise_prob)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or not 0.0 <= v <= 1.0:
            raise ValueError('%s: %s must be a probability in [0, 1], got %r' % (what, name, v))
        q24.append(int(round(v * (1 << 24))))
    try:
        lo, hi = snr
    except (TypeError, ValueError):
        raise ValueError('%s: snr must be a (low, high) pair in dB, got %r' % (what, snr))
    for v in (lo, hi):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or abs(v) > 3e38:
            raise ValueError('%s: the snr bounds must be finite numbers, got %r' % (what, snr))
    if lo > hi:
        raise ValueError('%s: need snr low <= snr high, got %r' % (what, snr))
    if isinstance(seed, bool) or not isinstance(seed, int):
        raise TypeError('%s: seed must be an integer, got %r' % (what, seed))
    if not 0 <= seed <= 0xFFFFFFFF:
        raise ValueError('%s: seed must fit 32 unsigned bits, got %d' % (what, seed))
    pol = L.NoiseReverbPolicy(rirs[0].shape[0] if rirs else 0, rirs[0].shape[1] if rirs else 1,
                              noises[0].shape[0] if noises else 0, noises[0].shape[1] if noises else 1,
                              q24[0], q24[1], float(lo), float(hi), seed)
    return rirs, noises, pol


def noise_reverb(wave, lengths, *, rirs=None, noises=None, rir_prob=1.0, noise_prob=1.0, snr=(5.0, 20.0), seed=0, counter=None,
                 return_plan=False):
    """Reverberation and additive noise for a batch of waveforms as two launches (qk_noise_reverb; semantics: include/qk.h,
    "Reverberation and additive noise").

    wave (B, n_max) int16 / float32 on the device; lengths (B,) valid samples per utterance (clamped to [0, n_max]).  rirs: a bank
    from prepare_rirs, or None; noises: a bank from prepare_noises, or None.  Per utterance, with probability rir_prob one response
    of the bank is drawn and the utterance convolved with it (aligned at the response's direct path, cut to the utterance's own
    length), and with probability noise_prob one recording is drawn, started at a drawn offset, wrapped around, and added at a
    signal-to-noise ratio drawn from [snr[0], snr[1]) dB against the (reverberated) utterance's energy.  The draws are a hash of
    (seed, counter, utterance): equal arguments give equal bits.  counter: one-element int32 / uint32 DEVICE tensor read by the
    kernel (None: 0).  Banks that live on another device are copied on every call: hand over device banks.

    Returns out (B, n_max) float32 at the input's scale, zero from lengths[b] on; lengths do not change.  With return_plan also plan
    (B, 8) int32 = {n, response or -1, recording or -1, offset, bits of the snr, bits of the noise gain, bits of float(signal
    energy), bits of float(noise energy)}.  No host sync."""
    what = 'noise_reverb'
    rirs, noises, pol = _env_args(what, rirs, noises, rir_prob, noise_prob, snr, seed)
    if torch.is_tensor(wave) and wave.dtype not in (torch.int16, torch.float32):
        raise TypeError('%s: waveforms must be int16 or float32, got %s' % (what, wave.dtype))
    if not torch.is_tensor(wave) or not wave.is_cuda:
        raise RuntimeError('%s: got a CPU tensor. Reverberation and additive noise run only on the MI355X HIP path (libqk_hip.so); '
                           'there is no CPU fallback.' % what)
    if wave.dim() != 2 or min(wave.shape) < 1:
        raise ValueError('%s: wave must be a non-empty (B, samples) tensor, got shape %s' % (what, tuple(wave.shape)))
    b, n_max = wave.shape
    lengths = lengths if torch.is_tensor(lengths) else torch.as_tensor(lengths)
    if lengths.numel() != b:
        raise ValueError('%s: lengths must have B = %d entries, got %d' % (what, b, lengths.numel()))
    lengths = lengths.reshape(-1).to(device=wave.device, dtype=torch.int32).contiguous()
    if counter is not None:
        if (not torch.is_tensor(counter) or counter.device != wave.device or counter.numel() != 1
                or counter.dtype not in (torch.int32, torch.uint32)):
            raise ValueError('%s: counter must be a one-element int32 / uint32 tensor on %s' % (what, wave.device))
    if n_max >= 1 << 26:
        raise ValueError('%s: rows of %d samples are not supported (limit 2^26)' % (what, n_max))
    rirs = tuple(t.to(wave.device).contiguous() for t in rirs) if rirs else (None, None, None)
    noises = tuple(t.to(wave.device).contiguous() for t in noises) if noises else (None, None)
    wave = wave.contiguous()
    out = torch.empty((b, n_max), dtype=torch.float32, device=wave.device)
    plan = torch.empty((b, L.QK_NOISE_REVERB_PLAN_WORDS), dtype=torch.int32, device=wave.device) if return_plan else None
    n = int(L.lib().qk_noise_reverb_workspace_bytes(b, n_max))
    ws = torch.empty(n // 8, dtype=torch.float64, device=wave.device)
    wd = L.QK_WAVE_I16 if wave.dtype == torch.int16 else L.QK_WAVE_F32
    with _on_device(wave.device):
        rc = L.lib().qk_noise_reverb(wd, b, n_max, _ptr(wave), _ptr(lengths), ctypes.byref(pol), _ptr(rirs[0]), _ptr(rirs[1]),
                                     _ptr(rirs[2]), _ptr(noises[0]), _ptr(noises[1]), _ptr(counter), _ptr(out), _ptr(plan), _ptr(ws), n,
                                     _stream(wave))
    L.check(rc, 'qk_noise_reverb')
    return (out, plan) if return_plan else out


# ---- Device-resident corpus (include/qk_data.h) ---------------------------------------------------------------------------------
CorpusArrays = collections.namedtuple('CorpusArrays', 'wave_pack wave_off wave_len label_pack label_off label_len aux_pack')
CorpusBatch = collections.namedtuple('CorpusBatch', 'wave lengths labels label_length aux utt plan')
_CORPUS_DTYPES = dict(wave_pack=torch.int16, wave_off=torch.int64, wave_len=torch.int32, label_pack=torch.int32, label_off=torch.int64,
                      label_len=torch.int32, aux_pack=torch.int32)


def _u32_arg(what, name, v):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= 0xFFFFFFFF:
        raise ValueError('%s: %s must be an integer in [0, 2^32), got %r' % (what, name, v))
    return int(v)


def _corpus_desc(what, corpus):
    """The checked qk_corpus_t of a CorpusArrays (data.DeviceCorpus.arrays) and the device it lives on."""
    if not isinstance(corpus, CorpusArrays):
        raise TypeError('%s: corpus_arrays must be a functional.CorpusArrays (data.DeviceCorpus.arrays), got %r' % (what, type(corpus)))
    if not torch.is_tensor(corpus.wave_pack) or not corpus.wave_pack.is_cuda:
        raise RuntimeError('%s: the corpus is not on a GPU. Batches are assembled only on the MI355X HIP path (libqk_hip.so); there '
                           'is no CPU fallback.' % what)
    dev = corpus.wave_pack.device
    for name, dtype in _CORPUS_DTYPES.items():
        t = getattr(corpus, name)
        if t is None and name == 'aux_pack':
            continue
        if not torch.is_tensor(t) or t.dtype != dtype or t.dim() != 1 or not t.is_contiguous() or t.device != dev:
            raise TypeError('%s: %s must be a contiguous 1-D %s tensor on %s' % (what, name, dtype, dev))
    num_utts = corpus.wave_len.numel()
    if num_utts < 1 or any(getattr(corpus, k).numel() != num_utts for k in ('wave_off', 'label_off', 'label_len')):
        raise ValueError('%s: wave_off, wave_len, label_off and label_len must have one entry per utterance (at least one)' % what)
    if corpus.wave_pack.numel() < 8 or corpus.wave_pack.numel() % 8 or corpus.wave_pack.data_ptr() % 16:
        raise ValueError('%s: wave_pack must hold a positive multiple of 8 samples and start on a 16-byte boundary' % what)
    if corpus.label_pack.numel() < 1 or (corpus.aux_pack is not None and corpus.aux_pack.numel() != corpus.label_pack.numel()):
        raise ValueError('%s: label_pack must hold at least one word, and aux_pack as many as label_pack' % what)
    desc = L.CorpusDesc(_ptr(corpus.wave_pack), _ptr(corpus.wave_off), _ptr(corpus.wave_len), _ptr(corpus.label_pack),
                        _ptr(corpus.label_off), _ptr(corpus.label_len), _ptr(corpus.aux_pack), corpus.wave_pack.numel(),
                        corpus.label_pack.numel(), num_utts, 0)
    return desc, dev


def corpus_batch(corpus_arrays, batches, position=0, cursor=None, seed=0, shuffle=False, *, n_out, l_out, aux=None, return_utt=False,
                 return_plan=False):
    """One batch of a device-resident corpus as one launch (qk_corpus_batch; semantics: include/qk_data.h).

    corpus_arrays: a CorpusArrays of device tensors (data.DeviceCorpus.arrays).  batches: (num_batches, batch) int32 DEVICE matrix of
    utterance indices; an index outside [0, num_utts) is an empty slot.  The batch is row `perm(seed, epoch, pos)` (shuffle) or
    `pos` of it, with epoch, pos = divmod(p, num_batches) and p = the value of `cursor` -- a one-element int32 / uint32 DEVICE
    tensor read by the kernel: advance it with a device op and a captured graph gathers a new batch on every replay -- or, without
    a cursor, `position`.  n_out / l_out: the widths of the padded waveform and label matrices; longer utterances are CUT (the
    callers in data.py refuse such widths before they launch).  aux: None = when the corpus has aux words.

    Returns a CorpusBatch: wave (batch, n_out) int16 zero-padded, lengths (batch,) int32, labels (batch, l_out) int32 zero-padded,
    label_length (batch,) int32, aux (batch, l_out) int32 padded with -1 or None, utt (batch,) int32 (-1: empty slot) or None,
    plan (4,) int32 = {p, epoch, pos, row} or None.  No host sync."""
    what = 'corpus_batch'
    desc, dev = _corpus_desc(what, corpus_arrays)
    if (not torch.is_tensor(batches) or batches.dtype != torch.int32 or batches.dim() != 2 or min(batches.shape) < 1
            or not batches.is_contiguous() or batches.device != dev):
        raise TypeError('%s: batches must be a non-empty contiguous (num_batches, batch) int32 tensor on %s' % (what, dev))
    position, seed = _u32_arg(what, 'position', position), _u32_arg(what, 'seed', seed)
    for name, v in (('n_out', n_out), ('l_out', l_out)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError('%s: %s must be an integer >= 1, got %r' % (what, name, v))
    if cursor is not None:
        if (not torch.is_tensor(cursor) or cursor.device != dev or cursor.numel() != 1 or cursor.dtype not in (torch.int32, torch.uint32)):
            raise ValueError('%s: cursor must be a one-element int32 / uint32 tensor on %s' % (what, dev))
    aux = corpus_arrays.aux_pack is not None if aux is None else bool(aux)
    if aux and corpus_arrays.aux_pack is None:
        raise ValueError('%s: aux=True, but the corpus has no aux words' % what)
    nb, b = batches.shape
    n_out, l_out = int(n_out), int(l_out)
    if b * n_out >= 1 << 31 or b * l_out >= 1 << 31:
        raise ValueError('%s: outputs of 2^31 elements or more are not supported (batch %d, n_out %d, l_out %d)' % (what, b, n_out, l_out))
    sched = L.BatchScheduleDesc(_ptr(batches), nb, b, seed, int(bool(shuffle)))
    wave = torch.empty((b, n_out), dtype=torch.int16, device=dev)
    lengths = torch.empty((b,), dtype=torch.int32, device=dev)
    labels = torch.empty((b, l_out), dtype=torch.int32, device=dev)
    label_length = torch.empty((b,), dtype=torch.int32, device=dev)
    aux_out = torch.empty((b, l_out), dtype=torch.int32, device=dev) if aux else None
    utt = torch.empty((b,), dtype=torch.int32, device=dev) if return_utt else None
    plan = torch.empty((L.QK_CORPUS_PLAN_WORDS,), dtype=torch.int32, device=dev) if return_plan else None
    with _on_device(dev):
        rc = L.lib().qk_corpus_batch(ctypes.byref(desc), ctypes.byref(sched), position, _ptr(cursor), n_out, l_out, _ptr(wave),
                                     _ptr(lengths), _ptr(labels), _ptr(label_length), _ptr(aux_out), _ptr(utt), _ptr(plan),
                                     _stream(wave))
    L.check(rc, 'qk_corpus_batch')
    return CorpusBatch(wave, lengths, labels, label_length, aux_out, utt, plan)


def epoch_permutation(seed, epoch, num_batches):
    """The order of one epoch, on the host (qk_epoch_permutation): a (num_batches,) int32 numpy array whose entry `pos` is the row
    of the schedule that position `pos` of epoch `epoch` reads under `seed`."""
    seed, epoch = _u32_arg('epoch_permutation', 'seed', seed), _u32_arg('epoch_permutation', 'epoch', epoch)
    if isinstance(num_batches, bool) or not isinstance(num_batches, (int, np.integer)) or not 1 <= num_batches < 1 << 31:
        raise ValueError('epoch_permutation: num_batches must be an integer in [1, 2^31), got %r' % (num_batches,))
    out = np.empty(int(num_batches), dtype=np.int32)
    L.check(L.lib().qk_epoch_permutation(seed, epoch, int(num_batches), out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))),
            'qk_epoch_permutation')
    return out


# ---- include/qk_rnn.h: the quaternion LSTM recurrence ----------------------------------------------------------------------------
def _aligned16(t):
    """t (or None) contiguous and 16-byte aligned: the recurrent kernels read 16-byte fragments."""
    if t is None:
        return None
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _seq_path(symbol, desc, names):
    """The name of the kernel family `symbol` (a qk_*_supported) reports for desc."""
    path = getattr(L.lib(), symbol)(ctypes.byref(desc))
    if path == 0:
        L.check(L.QK_ERR_INVALID_ARG, symbol)
    return names[path]


def _lengths_arg(what, lengths, batch, device):
    """lengths (or None) checked as an int32 (batch,) tensor on device, contiguous."""
    if lengths is None:
        return None
    if lengths.dtype != torch.int32 or tuple(lengths.shape) != (batch,) or lengths.device != device:
        raise ValueError('%s: lengths must be an int32 tensor of shape (%d,) on %s' % (what, batch, device))
    return lengths.contiguous()


def _bwd_workspace(symbol, desc, dev):
    """(bytes, uint8 tensor): the backward workspace `symbol` (a qk_*_workspace_bytes) asks for.  Call inside _on_device(dev)."""
    n = int(getattr(L.lib(), symbol)(ctypes.byref(desc), L.QK_OP_BWD))
    if n == 0:
        L.check(L.QK_ERR_INVALID_ARG, symbol)
    return n, torch.empty(n, dtype=torch.uint8, device=dev)


def qlstm_desc(dtype, batch, steps, q_units, directions, reverse=False):
    return L.QLSTMDesc(_DTYPES[dtype], int(batch), int(steps), int(q_units), int(directions), int(directions) * 4 * int(q_units),
                       L.QK_QLSTM_REVERSE if reverse else 0)


def qlstm_path(dtype, batch, steps, q_units, directions=1):
    """'mfma16' / 'generic': the kernel family qk_qlstm_fwd / qk_qlstm_bwd run for this shape (qk_qlstm_supported)."""
    return _seq_path('qk_qlstm_supported', qlstm_desc(dtype, batch, steps, q_units, directions), L.QK_QLSTM_PATH_NAMES)


class _QLSTMFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, zx, R, lengths, h0, c0, reverse):
        D, B, T, G = zx.shape
        U = G // 4
        desc = qlstm_desc(zx.dtype, B, T, U // 4, D, reverse)
        dev = zx.device
        y = torch.empty((B, T, D * U), dtype=zx.dtype, device=dev)
        hT = torch.empty((D, B, U), dtype=zx.dtype, device=dev)
        cT = torch.empty((D, B, U), dtype=torch.float32, device=dev)
        with _on_device(dev):
            lib = L.lib()
            n = int(lib.qk_qlstm_workspace_bytes(ctypes.byref(desc), L.QK_OP_FWD))
            nr = int(lib.qk_qlstm_reserve_bytes(ctypes.byref(desc)))
            if n == 0 or nr == 0:
                L.check(L.QK_ERR_INVALID_ARG, 'qk_qlstm_workspace_bytes')
            ws = torch.empty(n, dtype=torch.uint8, device=dev)
            reserve = torch.empty(nr, dtype=torch.uint8, device=dev)
            rc = lib.qk_qlstm_fwd(ctypes.byref(desc), _ptr(zx), _ptr(R), _ptr(lengths), _ptr(h0), _ptr(c0), _ptr(y), _ptr(hT), _ptr(cT),
                                  _ptr(reserve), _ptr(ws), n, _stream(zx))
        L.check(rc, 'qk_qlstm_fwd')
        ctx.desc, ctx.shape = desc, (D, B, T, U)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(R, lengths, h0, c0, y, reserve)
        return y, hT, cT

    @staticmethod
    def backward(ctx, dy, dhT, dcT):
        R, lengths, h0, c0, y, reserve = ctx.saved_tensors
        desc, (D, B, T, U) = ctx.desc, ctx.shape
        dev, dtype = y.device, y.dtype
        dy = _aligned16(dy) if dy is not None else torch.zeros((B, T, D * U), dtype=dtype, device=dev)
        dhT = _aligned16(dhT)
        dcT = dcT.contiguous() if dcT is not None else None
        dzx = torch.empty((D, B, T, 4 * U), dtype=dtype, device=dev)
        hprev = torch.empty((D, B, T, U), dtype=dtype, device=dev)
        dh0 = torch.empty((D, B, U), dtype=dtype, device=dev)
        dc0 = torch.empty((D, B, U), dtype=torch.float32, device=dev)
        with _on_device(dev):
            n, ws = _bwd_workspace('qk_qlstm_workspace_bytes', desc, dev)
            rc = L.lib().qk_qlstm_bwd(ctypes.byref(desc), _ptr(dy), _ptr(dhT), _ptr(dcT), _ptr(R), _ptr(lengths), _ptr(h0), _ptr(c0), _ptr(y),
                                      _ptr(reserve), _ptr(dzx), _ptr(hprev), _ptr(dh0), _ptr(dc0), _ptr(ws), n, _stream(dy))
        L.check(rc, 'qk_qlstm_bwd')
        dR = None
        if ctx.needs_input_grad[1]:
            # dR[d] = sum_t dense-weight-gradient(h_{t-1}, dz_t): ONE dense backward-weight over the stacked (B * T) rows per direction
            # (inactive rows hold dz = 0)
            call = dense_call((B * T, U), (U // 4, 4 * U), dtype, None, False)
            dR = torch.empty((D, U // 4, 4 * U), dtype=torch.float32, device=dev)
            for d in range(D):
                call.bwd_weight(hprev[d].view(B * T, U), dzx[d].view(B * T, 4 * U), None, False, out=(dR[d], None))
        return (dzx, dR, None, dh0 if ctx.needs_input_grad[3] else None, dc0 if ctx.needs_input_grad[4] else None, None)


def qlstm(zx, R, lengths=None, h0=None, c0=None, reverse=False):
    """The quaternion LSTM recurrence (include/qk_rnn.h): one launch per time step, both directions in each.

    zx       (D, B, T, 4 * units): the input projection quaternion_dense(x, W) + b of each direction, D = 1 or 2 -- or (B, T, 4 * units)
             for one direction, with R (q_units, 4 * units) and states (B, units)
    R        (D, q_units, 4 * units) float32: the recurrent weight, a QuaternionDense weight of 4 * units outputs (gates i|f|g|o)
    lengths  (B,) int32 or None: rows are inactive from t = lengths[b] on (state carried, y = 0, no gradient)
    h0, c0   (D, B, units) or None (zero): h0 in zx's dtype, c0 float32
    reverse  one direction only: walk t = T-1 .. 0 (direction 1 of a two-direction call always does)

    Returns (y, hT, cT): y (B, T, D * units) in zx's dtype -- component c, direction d, unit u at column c * (D * q_units) + d * q_units
    + u -- hT (D, B, units) in zx's dtype, cT (D, B, units) float32.  The backward returns dzx, dR, dh0, dc0."""
    _require_device(zx, 'qlstm')
    single = zx.dim() == 3
    if single:
        zx, R = zx.unsqueeze(0), R.unsqueeze(0)
        h0 = h0.unsqueeze(0) if h0 is not None else None
        c0 = c0.unsqueeze(0) if c0 is not None else None
    if zx.dim() != 4 or R.dim() != 3 or zx.shape[0] not in (1, 2) or zx.shape[-1] % 16:
        raise ValueError('qlstm: zx must be (D, B, T, 4 * units) with D in (1, 2) and units divisible by 4, got %s' % (tuple(zx.shape),))
    D, B, T, G = zx.shape
    U = G // 4
    if R.dtype != torch.float32 or tuple(R.shape) != (D, U // 4, 4 * U):
        raise ValueError('qlstm: R must be float32 of shape %s, got %s %s' % ((D, U // 4, 4 * U), R.dtype, tuple(R.shape)))
    if reverse and D != 1:
        raise ValueError('qlstm: reverse needs one direction')
    if B == 0 or T == 0:
        raise ValueError('qlstm: empty batch or sequence')
    lengths = _lengths_arg('qlstm', lengths, B, zx.device)
    for name, s, dt in (('h0', h0, zx.dtype), ('c0', c0, torch.float32)):
        if s is not None and (tuple(s.shape) != (D, B, U) or s.dtype != dt or s.device != zx.device):
            raise ValueError('qlstm: %s must be %s of shape %s on %s' % (name, dt, (D, B, U), zx.device))
    y, hT, cT = _QLSTMFn.apply(_aligned16(zx), R.contiguous(), lengths, _aligned16(h0), c0.contiguous() if c0 is not None else None,
                               bool(reverse))
    if single:
        hT, cT = hT[0], cT[0]
    return y, hT, cT


# ---- include/qk_norm.h: quaternion layer normalisation ---------------------------------------------------------------------------
def qlayer_norm_desc(dtype, rows, q, steps=0, x_stride=None, y_stride=None):
    """qk_qlnorm_desc_t for `rows` rows of 4 * q columns; strides in elements (default: dense rows)."""
    width = 4 * int(q)
    return L.QLNormDesc(_DTYPES[dtype], int(rows), int(steps), int(q), width if x_stride is None else int(x_stride),
                        width if y_stride is None else int(y_stride), 0)


def qlayer_norm_path(dtype, rows, q):
    """'vec' / 'generic': the kernel family qk_qlnorm_fwd / qk_qlnorm_bwd run for dense, 16-byte aligned rows of this shape
    (qk_qlnorm_supported)."""
    return _seq_path('qk_qlnorm_supported', qlayer_norm_desc(dtype, rows, q), L.QK_QLNORM_PATH_NAMES)


def _rows_of(t, width):
    """t (N, width) as the kernels take it: unit column stride and a row stride >= width (a column window stays a view)."""
    return t if t.stride(1) == 1 and (t.stride(0) >= width or t.shape[0] == 1) and t.stride(0) < 2 ** 31 else t.contiguous()


class _QLNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, lengths, steps, epsilon):
        N, W = x.shape
        x = _rows_of(x, W)
        desc = qlayer_norm_desc(x.dtype, N, W // 4, steps, max(x.stride(0), W), W)
        dev = x.device
        y = torch.empty((N, W), dtype=x.dtype, device=dev)
        stats = torch.empty((N, 5), dtype=torch.float32, device=dev)
        with _on_device(dev):
            rc = L.lib().qk_qlnorm_fwd(ctypes.byref(desc), _ptr(x), _ptr(gamma), _ptr(beta), _ptr(lengths), float(epsilon), _ptr(y),
                                       _ptr(stats), _stream(x))
        L.check(rc, 'qk_qlnorm_fwd')
        ctx.steps = steps
        ctx.save_for_backward(x, gamma, lengths, stats)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, lengths, stats = ctx.saved_tensors
        N, W = x.shape
        dev = x.device
        if x.stride(0) != W and N > 1:
            x = x.contiguous()                      # dx has x's row stride: a column window is gathered once here
        dy = _rows_of(dy, W)
        desc = qlayer_norm_desc(x.dtype, N, W // 4, ctx.steps, W, max(dy.stride(0), W))
        dx = torch.empty((N, W), dtype=x.dtype, device=dev)
        dgamma = torch.empty((W // 4,), dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
        dbeta = torch.empty((W,), dtype=torch.float32, device=dev) if ctx.needs_input_grad[2] else None
        with _on_device(dev):
            n, ws = (0, None) if dgamma is None and dbeta is None else _bwd_workspace('qk_qlnorm_workspace_bytes', desc, dev)
            rc = L.lib().qk_qlnorm_bwd(ctypes.byref(desc), _ptr(dy), _ptr(x), _ptr(gamma), _ptr(lengths), _ptr(stats), _ptr(dx),
                                       _ptr(dgamma), _ptr(dbeta), _ptr(ws), n, _stream(x))
        L.check(rc, 'qk_qlnorm_bwd')
        return dx, dgamma, dbeta, None, None, None


def qlayer_norm(x, gamma=None, beta=None, lengths=None, epsilon=1e-3):
    """Quaternion layer normalisation (include/qk_norm.h) of the last axis of x, (..., 4 Q) component-major r|i|j|k: per row the four
    component means are removed and ONE variance over all 4 Q values scales the row.

    gamma    (Q,) float32 or None: one scale per quaternion unit, shared by its four components
    beta     (4 Q,) float32 or None
    lengths  (B,) int32 or None, with x (B, T, 4 Q): rows with t >= lengths[b] are inactive -- y = 0 (not beta), no gradient
    Returns y in x's shape and dtype; the backward returns dx, dgamma, dbeta."""
    _require_device(x, 'qlayer_norm')
    if x.dim() < 1 or x.shape[-1] % 4 or x.numel() == 0:
        raise ValueError('qlayer_norm: x must be a non-empty (..., 4 Q) tensor, got %s' % (tuple(x.shape),))
    W = x.shape[-1]
    steps = 0
    if lengths is not None:
        if x.dim() != 3:
            raise ValueError('qlayer_norm: lengths needs x of shape (B, T, 4 Q), got %s' % (tuple(x.shape),))
        lengths, steps = _lengths_arg('qlayer_norm', lengths, x.shape[0], x.device), x.shape[1]
    for name, p, n in (('gamma', gamma, W // 4), ('beta', beta, W)):
        if p is not None and (p.dtype != torch.float32 or tuple(p.shape) != (n,) or p.device != x.device):
            raise ValueError('qlayer_norm: %s must be float32 of shape (%d,) on %s' % (name, n, x.device))
    y = _QLNormFn.apply(x.reshape(-1, W), _aligned16(gamma), _aligned16(beta), lengths, steps, float(epsilon))
    return y.view(x.shape)


# ---- include/qk_attn.h: quaternion multi-head self-attention --------------------------------------------------------------------
def qattention_desc(dtype, batch, steps, heads, dq, q=None, k=None, v=None, o=None):
    """qk_qattn_desc_t for (batch, steps, 4 * heads * dq) tensors; q, k, v, o are (row, comp) stride pairs in elements (default: dense
    rows of 4 Q columns, components Q apart)."""
    Q = int(heads) * int(dq)
    pairs = [(4 * Q, Q) if s is None else (int(s[0]), int(s[1])) for s in (q, k, v, o)]
    return L.QAttnDesc(_DTYPES[dtype], int(batch), int(steps), int(heads), int(dq), pairs[0][0], pairs[0][1], pairs[1][0], pairs[1][1],
                       pairs[2][0], pairs[2][1], pairs[3][0], pairs[3][1], 0)


def qattention_path(dtype, batch, steps, heads, dq, packed=False):
    """'mfma' / 'generic': the kernel family qk_qattn_fwd / qk_qattn_bwd run for dense (packed: (B, T, 12 Q)), 16-byte aligned tensors
    of this shape (qk_qattn_supported)."""
    Q = int(heads) * int(dq)
    s = (12 * Q, 3 * Q) if packed else None
    return _seq_path('qk_qattn_supported', qattention_desc(dtype, batch, steps, heads, dq, s, s, s, None), L.QK_QATTN_PATH_NAMES)


def _attn_rows(t, width):
    """t (B, T, width) as the attention kernels address it -- row b * T + t at (b * T + t) * row, unit column stride -- and its row
    stride in elements; a column window of a wider (B, T, W) buffer stays a view."""
    B, T, _ = t.shape
    row = t.stride(1) if T > 1 else (t.stride(0) if B > 1 else width)
    if t.stride(2) == 1 and width <= row < 2 ** 30 and (B == 1 or T == 1 or t.stride(0) == T * row):
        return t, row
    return t.contiguous(), width


def _qattn_fwd(dtype, B, T, heads, dq, strides, ptrs, lengths, scale, dev, stream_of):
    Q = heads * dq
    desc = qattention_desc(dtype, B, T, heads, dq, strides[0], strides[1], strides[2], None)
    o = torch.empty((B, T, 4 * Q), dtype=dtype, device=dev)
    lse = torch.empty((B, heads, T), dtype=torch.float32, device=dev)
    with _on_device(dev):
        rc = L.lib().qk_qattn_fwd(ctypes.byref(desc), ptrs[0], ptrs[1], ptrs[2], _ptr(lengths), float(scale), _ptr(o), _ptr(lse),
                                  _stream(stream_of))
    L.check(rc, 'qk_qattn_fwd')
    return o, lse


def _qattn_bwd(dtype, B, T, heads, dq, strides, ptrs, gptrs, do, o, lse, lengths, scale, dev):
    desc = qattention_desc(dtype, B, T, heads, dq, strides[0], strides[1], strides[2], None)
    with _on_device(dev):
        n, ws = _bwd_workspace('qk_qattn_workspace_bytes', desc, dev)
        rc = L.lib().qk_qattn_bwd(ctypes.byref(desc), _ptr(do), ptrs[0], ptrs[1], ptrs[2], _ptr(o), _ptr(lse), _ptr(lengths),
                                  float(scale), gptrs[0], gptrs[1], gptrs[2], _ptr(ws), n, _stream(do))
    L.check(rc, 'qk_qattn_bwd')


class _QAttnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, lengths, heads, scale):
        B, T, W = q.shape
        Q = W // 4
        views = [_attn_rows(t, W) for t in (q, k, v)]
        o, lse = _qattn_fwd(q.dtype, B, T, heads, Q // heads, [(r, Q) for _, r in views], [t.data_ptr() for t, _ in views], lengths,
                            scale, q.device, q)
        ctx.heads, ctx.scale = heads, scale
        ctx.save_for_backward(views[0][0], views[1][0], views[2][0], o, lse, lengths)
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse, lengths = ctx.saved_tensors
        B, T, W = o.shape
        Q = W // 4
        q, k, v, do = q.contiguous(), k.contiguous(), v.contiguous(), do.contiguous()      # the gradients are dense: so are their inputs
        grads = [torch.empty((B, T, W), dtype=o.dtype, device=o.device) for _ in range(3)]
        _qattn_bwd(o.dtype, B, T, ctx.heads, Q // ctx.heads, [(W, Q)] * 3, [q.data_ptr(), k.data_ptr(), v.data_ptr()],
                   [g.data_ptr() for g in grads], do, o, lse, lengths, ctx.scale, o.device)
        return grads[0], grads[1], grads[2], None, None, None


class _QAttnPackedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, lengths, heads, scale):
        B, T, W = qkv.shape
        Q = W // 12
        qkv, row = _attn_rows(qkv, W)
        es = qkv.element_size()
        ptrs = [qkv.data_ptr() + i * Q * es for i in range(3)]
        o, lse = _qattn_fwd(qkv.dtype, B, T, heads, Q // heads, [(row, 3 * Q)] * 3, ptrs, lengths, scale, qkv.device, qkv)
        ctx.heads, ctx.scale = heads, scale
        ctx.save_for_backward(qkv, o, lse, lengths)
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, o, lse, lengths = ctx.saved_tensors
        B, T, W = qkv.shape
        Q = W // 12
        qkv, do = qkv.contiguous(), do.contiguous()
        es = qkv.element_size()
        grad = torch.empty((B, T, W), dtype=qkv.dtype, device=qkv.device)       # ONE gradient: dq | dk | dv windows of every component
        _qattn_bwd(qkv.dtype, B, T, ctx.heads, Q // ctx.heads, [(W, 3 * Q)] * 3, [qkv.data_ptr() + i * Q * es for i in range(3)],
                   [grad.data_ptr() + i * Q * es for i in range(3)], do, o, lse, lengths, ctx.scale, qkv.device)
        return grad, None, None, None


def _qattn_check(what, x, width_mult, heads, lengths, scale):
    _require_device(x, what)
    heads = int(heads)
    if x.dim() != 3 or x.numel() == 0 or heads < 1 or x.shape[-1] % (width_mult * heads):
        raise ValueError('%s: needs a non-empty (B, T, %d Q) tensor with heads = %d dividing Q, got %s'
                         % (what, width_mult, heads, tuple(x.shape)))
    lengths = _lengths_arg(what, lengths, x.shape[0], x.device)
    if scale is None:
        scale = 0.0                                  # the library's default: 1 / sqrt(4 dq)
    elif not 0.0 < float(scale) < float('inf'):
        raise ValueError('%s: scale must be a positive finite number or None, got %r' % (what, scale))
    return heads, lengths, scale


def qattention(q, k, v, heads, lengths=None, scale=None):
    """Quaternion multi-head self-attention (include/qk_attn.h).  q, k, v: (B, T, 4 Q) component-major r|i|j|k with Q = heads * dq;
    head h owns units h * dq .. of every component.  o = softmax_{t' < n}(scale * <q_t, k_t'>) v over the 4 dq reals of a head, with
    n = lengths[b]; rows t >= n are inactive: o = 0 exactly, no gradient, and nothing in them is read.  scale None: 1 / sqrt(4 dq).
    Views with a unit column stride (column windows of a wider (B, T, W) buffer) are read in place.  Returns o (B, T, 4 Q); the
    backward returns dq, dk, dv."""
    heads, lengths, scale = _qattn_check('qattention', q, 4, heads, lengths, scale)
    for name, t in (('k', k), ('v', v)):
        if t.shape != q.shape or t.dtype != q.dtype or t.device != q.device:
            raise ValueError('qattention: %s must match q (%s %s on %s)' % (name, q.dtype, tuple(q.shape), q.device))
    return _QAttnFn.apply(q, k, v, lengths, heads, scale)


def qattention_packed(qkv, heads, lengths=None, scale=None):
    """qattention on the (B, T, 12 Q) output of ONE QuaternionDense with 3 Q quaternion units: component c holds q | k | v units at
    columns c * 3Q + [0, Q), [Q, 2Q), [2Q, 3Q), read in place through the component strides.  The backward writes ONE (B, T, 12 Q)
    gradient, so the projection's backward sees one dy and no cat."""
    heads, lengths, scale = _qattn_check('qattention_packed', qkv, 12, heads, lengths, scale)
    return _QAttnPackedFn.apply(qkv, lengths, heads, scale)


# ---- include/qk_dwconv.h: depthwise quaternion convolution over time with a fused GLU gate ----------------------------------------
def qdwconv_desc(dtype, batch, steps, units, taps, pad_lo, x=None, y=None):
    """qk_qdwconv_desc_t for (batch, steps, 4 * units) tensors; x, y are (row, comp) stride pairs in elements (default: dense rows of
    4 Q columns, components Q apart)."""
    Q = int(units)
    xs, ys = [(4 * Q, Q) if s is None else (int(s[0]), int(s[1])) for s in (x, y)]
    return L.QDWConvDesc(_DTYPES[dtype], int(batch), int(steps), Q, int(taps), int(pad_lo), xs[0], xs[1], ys[0], ys[1], 0)


def qdwconv_pad_lo(taps, padding):
    """Zeros in front of the sequence: 'same' (K - 1) // 2, 'causal' K - 1 (the convention of QuaternionConv1D)."""
    if padding == 'same':
        return (int(taps) - 1) // 2
    if padding == 'causal':
        return int(taps) - 1
    raise ValueError("padding must be 'same' or 'causal', got %r" % (padding,))


def qdwconv_path(dtype, batch, steps, units, taps=15, packed=False):
    """'vec' / 'generic': the kernel family qk_qdwconv_fwd / qk_qdwconv_bwd run for dense (packed: (B, T, 8 Q) gated input), 16-byte
    aligned tensors of this shape (qk_qdwconv_supported)."""
    Q = int(units)
    desc = qdwconv_desc(dtype, batch, steps, Q, taps, 0, (8 * Q, 2 * Q) if packed else None)
    return _seq_path('qk_qdwconv_supported', desc, L.QK_QDWCONV_PATH_NAMES)


def qdwconv_last_path():
    """'vec' / 'generic': what this thread's most recent depthwise call launched (qk_qdwconv_last_path)."""
    return L.QK_QDWCONV_PATH_NAMES[L.lib().qk_qdwconv_last_path()]


class _QDWConvFn(torch.autograd.Function):
    """x is (B, T, 4 Q), or with `gated` the packed (B, T, 8 Q): a | g inside every component."""

    @staticmethod
    def forward(ctx, x, kernel, bias, lengths, pad_lo, gated):
        B, T, W = x.shape
        Q = W // (8 if gated else 4)
        x, row = _attn_rows(x, W)
        comp = W // 4
        es = x.element_size()
        desc = qdwconv_desc(x.dtype, B, T, Q, kernel.shape[0], pad_lo, (row, comp))
        y = torch.empty((B, T, 4 * Q), dtype=x.dtype, device=x.device)
        with _on_device(x.device):
            rc = L.lib().qk_qdwconv_fwd(ctypes.byref(desc), x.data_ptr(), x.data_ptr() + Q * es if gated else None, _ptr(kernel),
                                        _ptr(bias), _ptr(lengths), _ptr(y), _stream(x))
        L.check(rc, 'qk_qdwconv_fwd')
        ctx.pad_lo, ctx.gated = pad_lo, gated
        ctx.save_for_backward(x, kernel, lengths)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, kernel, lengths = ctx.saved_tensors
        B, T, W = x.shape
        gated = ctx.gated
        Q = W // (8 if gated else 4)
        dev = x.device
        x = x.contiguous()                                  # the gradient is dense: so is its input
        dy, yrow = _attn_rows(dy, 4 * Q)
        es = x.element_size()
        desc = qdwconv_desc(x.dtype, B, T, Q, kernel.shape[0], ctx.pad_lo, (W, W // 4), (yrow, Q))
        grad = torch.empty((B, T, W), dtype=x.dtype, device=dev)      # gated: ONE gradient, da | dg windows of every component
        dw = torch.empty(tuple(kernel.shape), dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
        dbias = torch.empty((4 * Q,), dtype=torch.float32, device=dev) if ctx.needs_input_grad[2] else None
        with _on_device(dev):
            n, ws = (0, None) if dw is None and dbias is None else _bwd_workspace('qk_qdwconv_workspace_bytes', desc, dev)
            rc = L.lib().qk_qdwconv_bwd(ctypes.byref(desc), dy.data_ptr(), x.data_ptr(), x.data_ptr() + Q * es if gated else None,
                                        _ptr(kernel), _ptr(lengths), grad.data_ptr(), grad.data_ptr() + Q * es if gated else None,
                                        _ptr(dw), _ptr(dbias), _ptr(ws), n, _stream(x))
        L.check(rc, 'qk_qdwconv_bwd')
        return grad, dw, dbias, None, None, None


def _qdwconv(what, x, mult, kernel, bias, lengths, padding):
    _require_device(x, what)
    if x.dim() != 3 or x.numel() == 0 or x.shape[-1] % mult:
        raise ValueError('%s: needs a non-empty (B, T, %d Q) tensor, got %s' % (what, mult, tuple(x.shape)))
    Q = x.shape[-1] // mult
    if kernel.dim() != 2 or kernel.dtype != torch.float32 or kernel.shape[1] != 4 * Q or not 1 <= kernel.shape[0] <= 31 \
            or kernel.device != x.device:
        raise ValueError('%s: kernel must be float32 of shape (K, %d) with K in 1 .. 31 on %s, got %s %s'
                         % (what, 4 * Q, x.device, kernel.dtype, tuple(kernel.shape)))
    if bias is not None and (bias.dtype != torch.float32 or tuple(bias.shape) != (4 * Q,) or bias.device != x.device):
        raise ValueError('%s: bias must be float32 of shape (%d,) on %s' % (what, 4 * Q, x.device))
    lengths = _lengths_arg(what, lengths, x.shape[0], x.device)
    return _QDWConvFn.apply(x, kernel.contiguous(), bias.contiguous() if bias is not None else None, lengths,
                            qdwconv_pad_lo(kernel.shape[0], padding), mult == 8)


def qdwconv1d(x, kernel, bias=None, lengths=None, padding='same'):
    """Depthwise quaternion convolution over time (include/qk_dwconv.h).  x: (B, T, 4 Q) component-major r|i|j|k; kernel (K, 4 Q)
    float32, K quaternion taps per unit, component-major per tap; bias (4 Q,) float32 or None.  y[t] = bias + sum_k W[k] (x) x[t + k -
    pad_lo] per unit, the Hamilton product in the order of the convolution layers; nothing mixes units.  With n = lengths[b] the
    sequence is zero outside [0, n) whatever x holds there, and rows t >= n give y = 0 exactly and take no gradient.  padding: 'same'
    or 'causal'.  Views with a unit column stride are read in place.  The backward returns dx, dkernel, dbias."""
    return _qdwconv('qdwconv1d', x, 4, kernel, bias, lengths, padding)


def qglu_dwconv1d(u, kernel, bias=None, lengths=None, padding='same'):
    """qdwconv1d of the gated input a * sigmoid(g), on the packed (B, T, 8 Q) output of ONE QuaternionDense with 2 Q quaternion
    units: component c holds a | g at columns c * 2Q + [0, Q), [Q, 2Q), read in place through the component stride.  The gate is
    evaluated once per element inside the kernel; the backward writes ONE (B, T, 8 Q) gradient, so the projection's backward sees
    one dy and no cat.  Returns (B, T, 4 Q)."""
    return _qdwconv('qglu_dwconv1d', u, 8, kernel, bias, lengths, padding)
