"""Bit-packed relu / dropout mask (include/qk.h: qk_conv_fwd_post_bits / qk_conv_bwd_post_bits).

In a run of layers y = dropout(relu(pre)) the backward-data epilogue of the next layer needs `y > 0` only; the forward
epilogue that stores y writes that predicate as one bit per element (bit i of the bit tensor = flat channels-last element
i: byte i >> 3, bit i & 7) and the consumers read the bits instead of y.  The bit is the predicate the 16-bit-mask road
evaluates (y > 0 on the value widened to float), so both roads are compared with torch.equal: no tolerances anywhere."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 256


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def _mods():
    import qcnn_amd
    from qcnn_amd import _lib
    return qcnn_amd.functional, _lib


def _host_bits(y, nbytes):
    """The canonical bit tensor of y, packed on the host: bit i = (element i widened to float > 0), little-endian bits."""
    pred = (y.detach().float().cpu().reshape(-1) > 0).numpy()
    out = np.zeros(nbytes, dtype=np.uint8)
    packed = np.packbits(pred, bitorder='little')
    out[:packed.size] = packed
    return torch.from_numpy(out)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _body_call(F, B, H, W, cq, fq, dtype):
    return F.conv_call((B, H, W, 4 * cq), (3, 5, cq, 4 * fq), dtype, 2, 1, 'same', 'channels_last', 1, None, True, False)


def _tensors(dev, B, H, W, cq, fq, dtype, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(B, H, W, 4 * cq, device=dev, generator=g).to(dtype)
    w = torch.randn(3, 5, cq, 4 * fq, device=dev, generator=g) / (15 * cq) ** 0.5
    b = torch.randn(4 * fq, device=dev, generator=g) / 10
    dy = torch.randn(B, H, W, 4 * fq, device=dev, generator=g).to(dtype)
    return x, w, b, dy


# (cq, fq) on (B, 6, 50): lines shorter than a band (per-row decode, ragged last tiles); (1, 14, 200): 204-position padded
# lines (wave-uniform line state, bands that straddle two lines)
SHAPES = [(3, 6, 50, 32, 32), (3, 6, 50, 64, 32), (3, 6, 50, 32, 64), (3, 6, 50, 64, 64), (1, 14, 200, 32, 32), (1, 14, 200, 64, 64)]
SHAPE_IDS = ['%dx%dx%d_%dto%d' % s for s in SHAPES]


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'fp16'])
@pytest.mark.parametrize('rate', [0.3, 0.0])
@pytest.mark.parametrize('shape', SHAPES, ids=SHAPE_IDS)
def test_producer_writes_the_host_packing_of_its_own_y_and_nothing_else(shape, rate, dtype):
    F, L = _mods()
    dev = _dev()
    B, H, W, cq, fq = shape
    call = _body_call(F, B, H, W, cq, fq, dtype)
    x, w, b, _ = _tensors(dev, B, H, W, cq, fq, dtype, 5)
    post = F.PostOp(None, -1, rate, 1234)
    nb = call.mask_bits_bytes()
    numel = B * H * W * 4 * fq
    assert nb == (numel + 7) // 8 == ((numel + 7) // 8 + 15) // 16 * 16
    _, y_ref = call.fwd_post(x, w, b, post)
    assert L.last_path() == 'mfma16_band'
    buf = torch.full((GUARD + nb + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    y = torch.empty_like(y_ref)
    ws, n = call._ws(L.QK_OP_FWD, x, None)
    rc = L.lib().qk_conv_fwd_post_bits(ctypes.byref(call.desc), ctypes.byref(post.struct), _ptr(x), _ptr(w), _ptr(b), None, _ptr(y),
                                       ctypes.c_void_p(buf.data_ptr() + GUARD), _ptr(ws), n, _stream())
    L.check(rc, 'qk_conv_fwd_post_bits')
    torch.cuda.synchronize()
    assert L.last_path() == 'mfma16_band'
    assert torch.equal(y, y_ref)
    got = buf.cpu()
    assert bool((got[:GUARD] == 0xA5).all()) and bool((got[GUARD + nb:] == 0xA5).all())
    want = _host_bits(y, nb)
    assert torch.equal(got[GUARD:GUARD + nb], want)
    frac = float(np.unpackbits(want.numpy()).mean())
    assert 0.1 < frac < 0.6                                           # (a mask worth testing: neither empty nor full)


def _relu_dropout_like(dev, shape, dtype, seed):
    """An activation as a relu + dropout layer leaves it: about a third positive, the rest +0."""
    g = torch.Generator(device=dev).manual_seed(seed)
    v = torch.randn(shape, device=dev, generator=g)
    keep = torch.rand(shape, device=dev, generator=g) > 0.3
    return (torch.relu(v) * keep / 0.7).to(dtype)


def _both_roads(F, L, call, x, bits, dy, w, post_x):
    """(dx, dw, db) of qk_conv_bwd_post (x re-read as the mask) and of qk_conv_bwd_post_bits, deterministic weight gradients."""
    with L.debug_flags(L.QK_DBG_DETERMINISTIC):
        old = call.bwd_post(x, dy, w, True, post_x, None, None)
        path_old = L.last_path()
        new = call.bwd_post(x, dy, w, True, post_x, None, None, x_bits=bits)
        path_new = L.last_path()
    torch.cuda.synchronize()
    assert path_old == path_new
    return old, new, path_new


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'fp16'])
@pytest.mark.parametrize('shape', SHAPES, ids=SHAPE_IDS)
def test_band_consumer_equals_the_sixteen_bit_mask_road(shape, dtype):
    F, L = _mods()
    dev = _dev()
    B, H, W, cq, fq = shape
    call = _body_call(F, B, H, W, cq, fq, dtype)
    assert call.reads_mask_bits()
    _, w, _, dy = _tensors(dev, B, H, W, cq, fq, dtype, 6)
    x = _relu_dropout_like(dev, (B, H, W, 4 * cq), dtype, 7)
    nb = (x.numel() // 8 + 15) // 16 * 16
    bits = _host_bits(x, nb).to(dev)
    old, new, path = _both_roads(F, L, call, x, bits, dy, w, F.PostOp(None, -1, 0.3, 99))
    assert path == 'mfma16_band'
    assert torch.equal(new[0], old[0])
    assert torch.equal(new[1], old[1]) and torch.equal(new[2], old[2])
    assert float(old[0].float().abs().max()) > 0


def _special_values(dev, shape, dtype):
    """+0, -0, smallest positive subnormal and normal, NaN of both signs, +-inf and three ordinary values, value (c + 3 r) % 11 at
    channel c of row r: every channel position (lane half, piece, element) meets every value, on every residue of the row index."""
    if dtype == torch.bfloat16:
        pats = [0x0000, 0x8000, 0x0001, 0x0080, 0x7FC0, 0xFFC0, 0x7F80, 0xFF80, 0x3F80, 0xBF80, 0x3F00]
    else:
        pats = [0x0000, 0x8000, 0x0001, 0x0400, 0x7E00, 0xFE00, 0x7C00, 0xFC00, 0x3C00, 0xBC00, 0x3800]
    ch = shape[-1]
    rows = int(np.prod(shape[:-1]))
    r, c = np.meshgrid(np.arange(rows), np.arange(ch), indexing='ij')
    v = np.array(pats, dtype=np.uint16)[(c + 3 * r) % 11].astype(np.int16)
    return torch.from_numpy(v).reshape(shape).view(dtype).to(dev)


def _head_call(F, L, B, Fr, T, dtype):
    return F.conv_call((B, Fr, T, 256), (Fr, 1, 64, 256), dtype, 2, 1, 'valid', 'channels_last', 1, None, True, True,
                       L.QK_KERNEL_CHANNEL_MAJOR)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'fp16'])
@pytest.mark.parametrize('consumer', ['band', 'point'])
def test_special_values_land_where_the_sixteen_bit_mask_puts_them(consumer, dtype):
    F, L = _mods()
    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(8)
    if consumer == 'band':
        B, H, W, cq, fq = 3, 6, 50, 32, 32
        call = _body_call(F, B, H, W, cq, fq, dtype)
        _, w, _, dy = _tensors(dev, B, H, W, cq, fq, dtype, 9)
        xs = (B, H, W, 4 * cq)
    else:
        B, Fr, T = 2, 14, 20
        call = _head_call(F, L, B, Fr, T, dtype)
        w = torch.randn(64 * Fr, 256, device=dev, generator=g) / 30
        dy = torch.randn(B, 1, T, 256, device=dev, generator=g).to(dtype)
        xs = (B, Fr, T, 256)
    x = _special_values(dev, xs, dtype)
    nb = (x.numel() // 8 + 15) // 16 * 16
    bits = _host_bits(x, nb)
    # the host predicate on the patterns themselves: set for subnormal, normal, +inf and the positive ordinary values only
    first = np.unpackbits(bits.numpy()[:2], bitorder='little')[:11].tolist()
    assert first == [0, 0, 1, 1, 0, 0, 1, 0, 1, 0, 1]
    old, new, path = _both_roads(F, L, call, x, bits.to(dev), dy, w, F.PostOp(None, -1, 0.3, 99))
    assert path == ('mfma16_band' if consumer == 'band' else 'mfma16_point')
    # bit for bit (dx holds no NaN: dy is finite and the mask selects, it does not multiply)
    assert torch.equal(new[0].view(torch.int16), old[0].view(torch.int16))
    kept = (new[0].float() != 0).cpu().reshape(-1).numpy()
    allowed = np.unpackbits(bits.numpy(), bitorder='little')[:kept.size].astype(bool)
    assert not bool((kept & ~allowed).any()) and kept.any()


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'fp16'])
def test_point_consumer_head_form_equals_the_sixteen_bit_mask_road(dtype):
    """(B, F, T, 4 x 64) under the (14, 1) 'valid' conj kernel in channel-major order, 64 output channels: 40 gathered rows in a
    128-row tile, so most of the tile's rows lie past the end."""
    F, L = _mods()
    dev = _dev()
    B, Fr, T = 2, 14, 20
    call = _head_call(F, L, B, Fr, T, dtype)
    assert call.reads_mask_bits() and call.mask_bits_bytes() == 0
    g = torch.Generator(device=dev).manual_seed(10)
    w = torch.randn(64 * Fr, 256, device=dev, generator=g) / 30
    dy = torch.randn(B, 1, T, 256, device=dev, generator=g).to(dtype)
    x = _relu_dropout_like(dev, (B, Fr, T, 256), dtype, 11)
    nb = (x.numel() // 8 + 15) // 16 * 16
    buf = torch.full((GUARD + nb + GUARD,), 0, dtype=torch.uint8, device=dev)
    bits = buf[GUARD:GUARD + nb]
    bits.copy_(_host_bits(x, nb))
    old, new, path = _both_roads(F, L, call, x, bits, dy, w, F.PostOp(None, -1, 0.3, 99))
    assert path == 'mfma16_point'
    assert torch.equal(new[0], old[0])
    assert torch.equal(new[1], old[1]) and torch.equal(new[2], old[2])
    assert float(old[0].float().abs().max()) > 0


def _model_step(dev, flags, L, frames):
    from qcnn_amd.models import TimitQCNN
    np.random.seed(51); torch.manual_seed(51)
    model = TimitQCNN(num_layers=10, start_filter=32, dropout=0.3, l2=1e-5)
    model.train()
    g = torch.Generator(device=dev).manual_seed(52)
    x = torch.randn(2, 4, 41, frames, device=dev, generator=g).to(torch.bfloat16)
    with torch.no_grad():
        model.eval(); model(x); model.train()                         # builds the parameters (same draws in both runs)
    dp = torch.randn(2, frames, 62, device=dev, generator=g)
    torch.manual_seed(53)                                             # the dropout base of THE step
    with L.debug_flags(L.QK_DBG_DETERMINISTIC | flags):
        loss = (model(x).float() * dp).sum() + model.regularization_loss()
        loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize('frames', [20, 52])
def test_model_step_is_the_same_with_and_without_mask_bits(monkeypatch, frames):
    """TimitQCNN(10 layers, start_filter 32, dropout 0.3, l2 1e-5), training mode, bf16, batch 2, deterministic gradients: one step
    from the same seeds with and without QK_DBG_NO_MASK_BITS.  At 20 frames a padded line is 24 positions, under the band kernels'
    48-position floor, so the body runs the general kernel and no link carries bits; 52 frames is the shortest input at which all
    ten body layers write them (nine band consumers and the head's point kernel)."""
    F, L = _mods()
    dev = _dev()
    used = []
    cls = type(_body_call(F, 1, 2, 8, 32, 32, torch.bfloat16))
    real = cls.fwd_post

    def spy(self, *a, **kw):
        used.append(kw.get('bits_bytes', 0))
        return real(self, *a, **kw)
    monkeypatch.setattr(cls, 'fwd_post', spy)
    loss_b, grads_b = _model_step(dev, 0, L, frames)
    with_bits = [u for u in used if u]
    del used[:]
    loss_o, grads_o = _model_step(dev, L.QK_DBG_NO_MASK_BITS, L, frames)
    assert len(with_bits) == (10 if frames == 52 else 0) and not any(used)       # (none with the switch set)
    assert torch.equal(loss_b, loss_o)
    assert grads_b.keys() == grads_o.keys() and len(grads_b) > 20
    for n in grads_b:
        assert torch.equal(grads_b[n], grads_o[n]), n


@pytest.mark.parametrize('odd', ['16to32', '48to48', 'stride2'])
def test_layers_without_a_bit_kernel_keep_the_old_road(odd):
    F, L = _mods()
    dev = _dev()
    dtype = torch.bfloat16
    B, H, W = 2, 6, 50
    widths = {'16to32': [32, 16, 32, 32], '48to48': [32, 48, 48, 32], 'stride2': [32, 32, 32, 32]}[odd]
    g = torch.Generator(device=dev).manual_seed(12)
    x = torch.randn(B, H, W, 4 * widths[0], device=dev, generator=g).to(dtype).requires_grad_(True)
    layers = []
    for i in range(3):
        cq, fq = widths[i], widths[i + 1]
        w = (torch.randn(3, 5, cq, 4 * fq, device=dev, generator=g) / (15 * cq) ** 0.5).requires_grad_(True)
        b = (torch.randn(4 * fq, device=dev, generator=g) / 10).requires_grad_(True)
        kw = dict(strides=(1, 2) if (odd == 'stride2' and i == 1) else 1, padding='same')
        kw['post'] = dict(alpha=None, rate=0.3, seed=70 + i)
        layers.append((w, b, kw))
    # the odd layer is layer 1: it neither writes bits nor reads those of layer 0
    sp = (B, H, W)
    odd_call = F.conv_call(sp + (4 * widths[1],), (3, 5, widths[1], 4 * widths[2]), dtype, 2, layers[1][2]['strides'], 'same',
                           'channels_last', 1, None, True, False)
    assert odd_call.mask_bits_bytes() == 0
    assert not odd_call.reads_mask_bits()

    def run(flags):
        for t in [x] + [p for l in layers for p in l[:2]]:
            t.grad = None
        with L.debug_flags(L.QK_DBG_DETERMINISTIC | flags):
            y = F.quaternion_conv_chain(x, layers)
            (y.float() ** 2).sum().backward()
        torch.cuda.synchronize()
        return [y.detach().clone(), x.grad.clone()] + [p.grad.clone() for l in layers for p in l[:2]]
    a, c = run(0), run(L.QK_DBG_NO_MASK_BITS)
    for p, q in zip(a, c):
        assert torch.equal(p, q)
    # the direct call says so instead of taking another road
    post = F.PostOp(None, -1, 0.3, 1)
    xin = torch.zeros(odd_call.x_shape, dtype=dtype, device=dev)
    with pytest.raises(RuntimeError, match='status -2'):
        odd_call.fwd_post(xin, layers[1][0].detach(), layers[1][1].detach(), post, bits_bytes=64)
