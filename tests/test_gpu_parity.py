"""GPU parity: the HIP path (through the C-ABI, via qcnn_amd.functional) against
  (1) the committed golden fixtures generated from the reference's own layer code, and
  (2) the CPU oracle on seeded inputs at sizes the oracle finishes in seconds.

Tolerances (stated per BASELINE.json north_star: fwd/bwd within 1e-4 relative, fp32):
  fp32 : max|got-want| <= 1e-4 * max|want|        (observed ~1e-6: the fp32 MFMA is an fmaf chain);
         for relu layers the backward is compared on the GPU's own relu mask (outputs that are zero up
         to rounding may land on either side of 0; the number of such sign differences is bounded)
  bf16 : x, kernel and dy are rounded to bf16 first and the oracle runs on the ROUNDED values in float64;
         16-bit outputs (y, dx) carry one bf16 rounding -> 1e-2 * max|want|; fp32 outputs
         (dkernel, dbias) -> 2e-3 (y feeding the relu mask is itself bf16-rounded)
  fp16 : same scheme, 2e-3 / 1e-3.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import golden_layer_files, layer_kwargs, load_golden

pytestmark = pytest.mark.gpu

FILES = golden_layer_files()
IDS = [os.path.basename(f)[:-4] for f in FILES]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def _rel_err(got, want):
    want = np.asarray(want, dtype=np.float64)
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.abs(got - want).max()) / max(float(np.abs(want).max()), 1e-30)


def _run_native(F, rec_x, rec_w, rec_b, rec_dy, rank, kw, dtype):
    """The native layout on a case: a channels_last convolution goes in its channels_first form (the same numbers, channel
    axis moved) through internal_layout='native', and y / dx come back channels_last; a dense layer has no layout."""
    if rank == 0 or kw.get('data_format', 'channels_last') == 'channels_first':
        return _run_layer(F, rec_x, rec_w, rec_b, rec_dy, rank, kw, dtype, 'native')
    got = _run_layer(F, np.moveaxis(rec_x, -1, 1), rec_w, rec_b, np.moveaxis(rec_dy, -1, 1), rank,
                     dict(kw, data_format='channels_first'), dtype, 'native')
    got['y'], got['dx'] = np.moveaxis(got['y'], 1, -1), np.moveaxis(got['dx'], 1, -1)
    return got


def _run_layer(F, rec_x, rec_w, rec_b, rec_dy, rank, kw, dtype, internal_layout='channels_last'):
    dev = _dev()
    x = torch.tensor(rec_x, device=dev).to(dtype).requires_grad_(True)
    w = torch.tensor(rec_w, device=dev, dtype=torch.float32).requires_grad_(True)
    b = None
    if rec_b is not None:
        b = torch.tensor(rec_b, device=dev, dtype=torch.float32).requires_grad_(True)
    if rank == 0:
        y = F.quaternion_dense(x, w, b, activation=kw['activation'])
    else:
        y = F.quaternion_conv(x, w, b, internal_layout=internal_layout, **kw)
    dy = torch.tensor(rec_dy, device=dev).to(dtype)
    y.backward(dy)
    torch.cuda.synchronize()
    out = dict(y=y.detach().float().cpu().numpy(), dx=x.grad.float().cpu().numpy(),
               dkernel=w.grad.cpu().numpy())
    if b is not None:
        out['dbias'] = b.grad.cpu().numpy()
    return out


@pytest.mark.parametrize('layout', ['channels_last', 'native'])
@pytest.mark.parametrize('path', FILES, ids=IDS)
def test_fp32_matches_reference_golden(path, layout):
    import qcnn_amd
    rec, cfg = load_golden(path)
    rank, kw = layer_kwargs(cfg)
    run = _run_native if layout == 'native' else _run_layer
    got = run(qcnn_amd.functional, rec['x'], rec['kernel'], rec.get('bias'), rec['dy'], rank, kw, torch.float32)
    for k, v in got.items():
        err = _rel_err(v, rec[k])
        assert err <= 1e-4, '%s: rel err %.3g' % (k, err)


def _oracle_case(rank, x_shape, w_shape, kw, seed, dtype=torch.float32, use_bias=True):
    from oracle import oracle
    rng = np.random.RandomState(seed)
    x = rng.randn(*x_shape).astype(np.float32)
    w = (rng.randn(*w_shape) / np.sqrt(np.prod(w_shape[:-1]) * 4)).astype(np.float32)
    b = (0.1 * rng.randn(w_shape[-1])).astype(np.float32) if use_bias else None
    if dtype != torch.float32:
        # 16-bit compute rounds activations AND the kernel to the 16-bit type (fp32 accumulate);
        # make both exactly representable so GPU and oracle see identical operands (otherwise
        # the relu mask of near-zero outputs differs and single flipped positions dominate dx)
        x = torch.tensor(x).to(dtype).float().numpy()
        w = torch.tensor(w).to(dtype).float().numpy()
    y = oracle.forward(x, w, b, rank, **kw)
    dy = rng.randn(*y.shape).astype(np.float32)
    if dtype != torch.float32:
        dy = torch.tensor(dy).to(dtype).float().numpy()
        # the GPU masks relu' with ITS y (rounded to 16 bit); positions where the rounding
        # flips the sign of a ~0 output are excluded by construction: y==0 after rounding only
        # if |y| underflows, which cannot happen at these magnitudes.
    dx, dw, db = oracle.backward(x, w, b, dy, rank, y=y, **kw)
    want = dict(y=y, dx=dx, dkernel=dw)
    if use_bias:
        want['dbias'] = db
    return x, w, b, dy, want


ORACLE_CASES = [
    # id, rank, x_shape, w_shape, kwargs
    ('cfg2_conv1d_b8_f64', 1, (8, 200, 160), (3, 40, 256),
     dict(padding='same', activation='relu')),
    ('cfg2_conv1d_b64_f32', 1, (64, 200, 160), (3, 40, 128),
     dict(padding='same', activation='relu')),
    # BASELINE config 2 exactly as benched (batch 64, 64 filters): the oracle needs ~8 s for it
    ('cfg2_conv1d_b64_f64_full', 1, (64, 200, 160), (3, 40, 256),
     dict(padding='same', activation='relu')),
    ('conv1d_odd_channels', 1, (5, 37, 28), (5, 7, 36),
     dict(padding='same', strides=2, activation='relu')),
    ('conv2d_body_small', 2, (2, 14, 40, 128), (3, 5, 32, 128),
     dict(padding='same', activation='relu')),
    ('conv2d_body64_small', 2, (1, 14, 40, 256), (3, 5, 64, 256),
     dict(padding='same', activation='relu')),
    ('conv2d_32to64', 2, (1, 9, 33, 128), (3, 3, 32, 256),
     dict(padding='same', activation='relu')),
    ('conv1d_64to32_valid', 1, (3, 70, 256), (5, 64, 128),
     dict(padding='valid', activation=None)),
    ('conv2d_chfirst_body_small', 2, (2, 128, 14, 40), (3, 5, 32, 128),
     dict(padding='same', activation='relu', data_format='channels_first')),
    ('conv2d_first_layer', 2, (3, 4, 41, 50), (3, 5, 1, 128),
     dict(padding='same', activation='relu', data_format='channels_first')),
    ('conv2d_stride_dil', 2, (2, 19, 23, 16), (3, 2, 4, 48),
     dict(padding='same', strides=(2, 1), activation=None)),
    ('conv3d_small', 3, (2, 6, 7, 5, 16), (2, 3, 2, 4, 32),
     dict(padding='same', activation='relu')),
    ('conv3d_32ch', 3, (1, 4, 5, 40, 128), (2, 3, 3, 32, 128),
     dict(padding='same', activation='relu')),
    ('conv2d_32ch_outer_stride_dil', 2, (2, 19, 40, 128), (3, 3, 32, 128),
     dict(padding='same', strides=(2, 1), activation='relu')),
    ('conv2d_64ch_valid_wide', 2, (1, 6, 70, 256), (3, 5, 64, 128),
     dict(padding='valid', activation=None)),
    # 16 quaternion channels -> 64 filters, five inner taps, lines longer than a K step (the band backward-weight's carried row
    # offsets): masked = the one-column-tile-per-wave instantiation that replaced the spilling <2,5,true> (round 4); linear = <2,5,false>
    ('conv2d_cq16_f64_5tap_relu', 2, (2, 5, 70, 64), (3, 5, 16, 256), dict(padding='same', activation='relu')),
    ('conv2d_cq16_f64_5tap_linear', 2, (2, 5, 70, 64), (3, 5, 16, 256), dict(padding='same', activation=None)),
    # round 5: channel counts that are multiples of 16 but not of 32 (start_filter = 16 models) -- the PAD forms of the 16-bit band
    # kernels (re-laid-out kernel zero-padded to 32, out-of-range DMA lanes, unstored output pieces): 16 -> 16, 16 -> 32, a
    # 48-channel layer whose second chunk is half real, a 1-D three-tap layer, and a relu layer (masked backward: fp32-MFMA forms)
    # (three inner taps, 64-filter blocks, no mask: four dY planes on six staging slots -- the first schedule of round 5 left the
    #  fourth plane out and no case saw it)
    ('conv2d_32to64_3tap_linear', 2, (1, 9, 70, 128), (3, 3, 32, 256), dict(padding='same', activation=None)),
    ('conv1d_16to64_3tap_linear', 1, (3, 150, 64), (3, 16, 256), dict(padding='same', activation=None)),
    # the pipelined band loop's corners: ONE group per tile (1-D, one 32-channel chunk: the second half of the two-group trip never runs),
    # two outer taps (an even group count with a single chunk), a 'valid' 5-tap 2-D layer whose tiles end inside an image line
    ('conv1d_32to32_5tap', 1, (3, 150, 128), (5, 32, 128), dict(padding='same', activation='relu')),
    ('conv2d_2x3_64ch', 2, (1, 6, 70, 256), (2, 3, 64, 256), dict(padding='same', activation=None)),
    ('conv2d_32to64_valid_5tap', 2, (2, 5, 61, 128), (3, 5, 32, 256), dict(padding='valid', activation='relu')),
    ('conv2d_16to16_5tap', 2, (2, 6, 80, 64), (3, 5, 16, 64), dict(padding='same', activation=None)),
    ('conv2d_16to16_5tap_relu', 2, (2, 6, 80, 64), (3, 5, 16, 64), dict(padding='same', activation='relu')),
    ('conv2d_16to32_3tap', 2, (2, 5, 75, 64), (3, 3, 16, 128), dict(padding='same', activation=None)),
    ('conv2d_48to16_5tap', 2, (1, 4, 90, 192), (3, 5, 48, 64), dict(padding='same', activation=None)),
    ('conv1d_16to48_valid', 1, (3, 100, 64), (3, 16, 192), dict(padding='valid', activation=None)),
    # one tap per produced row: the streaming point-form kernel (k_hgemm16_point) in 16 bit
    ('dense_point_64', 0, (333, 256), (64, 256), dict(activation='relu')),
    ('dense_point_32to128', 0, (200, 128), (32, 512), dict(activation=None)),
    # produced widths of 32 channels per component: the point form's 32-channel column blocks (256-row tiles) -- a dense layer, a 1 x 1
    # convolution and the backward-data of a 32 -> 64 head (start_filter = 16 models)
    ('dense_point_64to32', 0, (300, 256), (64, 128), dict(activation='relu')),
    ('conv1d_1x1_32to32', 1, (3, 101, 128), (1, 32, 128), dict(padding='same', activation=None)),
    ('conv2d_head_valid_conj_32to64', 2, (3, 6, 50, 128), (6, 1, 32, 256), dict(padding='valid', activation=None, conj=True)),
    ('conv2d_head_valid_conj', 2, (3, 6, 50, 256), (6, 1, 64, 256), dict(padding='valid', activation=None, conj=True)),
    ('conv1d_1x1_64', 1, (4, 77, 256), (1, 64, 256), dict(padding='same', activation='relu')),
    ('dense_qdnn0', 0, (32, 1000), (250, 512), dict(activation='relu')),
    ('dense_timit_head', 0, (300, 3584), (896, 256), dict(activation='relu')),
    ('dense_wide', 0, (130, 512), (128, 1024), dict(activation=None)),
]


@pytest.mark.parametrize('case', ORACLE_CASES, ids=[c[0] for c in ORACLE_CASES])
def test_fp32_matches_oracle(case):
    import qcnn_amd
    _, rank, xs, ws, kw = case
    x, w, b, dy, want = _oracle_case(rank, xs, ws, kw, seed=7)
    got = _run_layer(qcnn_amd.functional, x, w, b, dy, rank, kw, torch.float32)
    assert _rel_err(got['y'], want['y']) <= 1e-4
    if kw.get('activation') == 'relu':
        # The gradients depend on the relu mask, i.e. on the SIGN of outputs that are zero up to rounding:
        # among millions of outputs a handful (|y| ~ 1e-7) come out on the other side of zero in float32
        # than in the float64 oracle, and each such element moves dx by one full dy*w term (2.6 % of
        # max|dx| at the full config-2 size).  The forward is compared above; the backward is compared
        # on the SAME mask -- the oracle's backward run with the GPU's y.
        from oracle import oracle
        flipped = int(((got['y'] > 0) != (want['y'] > 0)).sum())
        assert flipped <= max(4, got['y'].size // 100000), 'relu mask differs in %d outputs' % flipped
        dx, dw, db = oracle.backward(x, w, b, dy, rank, y=got['y'].astype(np.float64), **kw)
        want = dict(want, dx=dx, dkernel=dw, dbias=db)
    for k, v in got.items():
        err = _rel_err(v, want[k])
        assert err <= 1e-4, '%s: rel err %.3g' % (k, err)


HALF_CASES = [c for c in ORACLE_CASES if c[0] in (
    'cfg2_conv1d_b8_f64', 'conv1d_odd_channels', 'conv2d_body_small', 'conv2d_body64_small', 'conv2d_32to64', 'conv1d_64to32_valid',
    'conv2d_chfirst_body_small',
    'conv2d_first_layer', 'dense_timit_head', 'dense_point_64', 'dense_point_32to128', 'conv2d_head_valid_conj', 'conv1d_1x1_64', 'conv3d_32ch', 'conv2d_32ch_outer_stride_dil', 'conv2d_64ch_valid_wide',
    'conv2d_cq16_f64_5tap_relu', 'conv2d_cq16_f64_5tap_linear',
    'conv2d_32to64_3tap_linear', 'conv1d_16to64_3tap_linear', 'conv2d_16to16_5tap', 'conv2d_16to16_5tap_relu', 'conv2d_16to32_3tap', 'conv2d_48to16_5tap', 'conv1d_16to48_valid',
    'conv1d_32to32_5tap', 'conv2d_2x3_64ch', 'conv2d_32to64_valid_5tap', 'dense_point_64to32', 'conv1d_1x1_32to32', 'conv2d_head_valid_conj_32to64')]


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'fp16'])
@pytest.mark.parametrize('case', HALF_CASES, ids=[c[0] for c in HALF_CASES])
def test_half_matches_oracle_on_rounded_inputs(case, dtype):
    import qcnn_amd
    _, rank, xs, ws, kw = case
    x, w, b, dy, want = _oracle_case(rank, xs, ws, kw, seed=11, dtype=dtype)
    got = _run_layer(qcnn_amd.functional, x, w, b, dy, rank, kw, dtype)
    tol16, tol32 = (1e-2, 2e-3) if dtype == torch.bfloat16 else (2e-3, 1e-3)
    for k, v in got.items():
        err = _rel_err(v, want[k])
        tol = tol16 if k in ('y', 'dx') else tol32
        assert err <= tol, '%s: rel err %.3g > %.1g' % (k, err, tol)


AB_SWITCH_CASES = [c for c in ORACLE_CASES if c[0] in (
    'conv2d_body_small', 'conv2d_body64_small', 'conv2d_32to64', 'conv2d_32to64_3tap_linear', 'conv2d_head_valid_conj', 'conv1d_64to32_valid')]


@pytest.mark.parametrize('switch', ['QK_DBG_BAND16_8WAVES', 'QK_DBG_WGRAD_BAND_V1', 'QK_DBG_NO_BAND16', 'QK_DBG_WGRAD16_ONE_TAP',
                                    'QK_DBG_NO_WGRAD_BAND', 'QK_DBG_NO_POINT16'])
@pytest.mark.parametrize('case', AB_SWITCH_CASES, ids=[c[0] for c in AB_SWITCH_CASES])
def test_ab_switch_kernels_match_oracle(case, switch):
    """Every A/B switch of include/qk.h selects kernels the default dispatch no longer reaches (the 8-wave band tilings, the
    round-2..4 backward-weight band kernel, the general implicit-GEMM forms under the band / point kernels, one-tap backward-weight
    blocks): they are what the committed A/B profiles were measured against, so they are held to the oracle like the defaults."""
    import qcnn_amd
    from qcnn_amd import _lib
    _, rank, xs, ws, kw = case
    dtype = torch.bfloat16
    x, w, b, dy, want = _oracle_case(rank, xs, ws, kw, seed=13, dtype=dtype)
    with _lib.debug_flags(getattr(_lib, switch)):
        got = _run_layer(qcnn_amd.functional, x, w, b, dy, rank, kw, dtype)
    for k, v in got.items():
        err = _rel_err(v, want[k])
        tol = 1e-2 if k in ('y', 'dx') else 2e-3
        assert err <= tol, '%s under %s: rel err %.3g > %.1g' % (k, switch, err, tol)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'fp16'])
def test_sixteen_channel_layers_run_on_the_matrix_cores(dtype):
    """/root/reference/models/interspeech_model.py:46-50: start_filter is a free hyperparameter; sf = 16 gives 16 -> 16 and 16 -> 32
    body layers.  Until round 5 every 16-bit call with Cq % 32 or F % 32 ran the fp32-MFMA kernels (1/16 of the bf16 rate); now
    multiples of 16 take the PAD forms of the band kernels in all three directions (qk_last_path), and the values are those
    of the exact fp32-MFMA kernels on the same rounded operands."""
    import qcnn_amd
    from qcnn_amd import _lib
    F = qcnn_amd.functional
    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(3)
    for cq, fq in ((16, 16), (16, 32), (32, 16), (48, 48)):
        xs, ws = (3, 7, 90, 4 * cq), (3, 5, cq, 4 * fq)
        x = torch.randn(xs, device=dev, generator=g).to(dtype)
        w = (torch.randn(ws, device=dev, generator=g) / 20).to(dtype).float()
        b = torch.randn(4 * fq, device=dev, generator=g) / 10
        call = F.conv_call(xs, ws, dtype, 2, 1, 'same', 'channels_last', 1, None, True, False)
        y = call.fwd(x, w, b)
        p_f = _lib.last_path()
        dy = torch.randn(y.shape, device=dev, generator=g).to(dtype)
        dx = call.bwd_data(dy, None, w)
        p_d = _lib.last_path()
        dw, db = call.bwd_weight(x, dy, None, True)
        p_w = _lib.last_path()
        # forward / backward-data: the streaming small-channel kernel where both widths are 16 or 32 (k_hconv16_small), the PAD form of
        # the band kernel elsewhere (48 channels); backward-weight: the LDS-DMA band kernel (16 x 32 blocks / PAD)
        small = lambda q, j: 'mfma16_small' if (q in (16, 32) and j == 16) else 'mfma16_band'       # (gathered, produced) channels per component
        assert (p_f, p_d, p_w) == (small(cq, fq), small(fq, cq), 'mfma16_band'), (cq, fq, p_f, p_d, p_w)
        with _lib.debug_flags(_lib.QK_DBG_NO_MFMA16):
            y0 = call.fwd(x, w, b)
            dx0 = call.bwd_data(dy, None, w)
            dw0, db0 = call.bwd_weight(x, dy, None, True)
            assert _lib.last_path() == 'fp32_mfma'
        tol = 1e-2 if dtype == torch.bfloat16 else 2e-3
        rel = lambda a, r: float((a.float() - r.float()).abs().max() / r.float().abs().max())
        assert rel(y, y0) <= tol and rel(dx, dx0) <= tol, (cq, fq, rel(y, y0), rel(dx, dx0))
        assert rel(dw, dw0) <= 1e-4 and rel(db, db0) <= 1e-4, (cq, fq, rel(dw, dw0), rel(db, db0))


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'fp16'])
def test_dense_weight_read_in_place_as_a_channel_major_kernel(dtype):
    """qk_conv_desc_t.kernel_order = QK_KERNEL_CHANNEL_MAJOR (round 6): the TIMIT model's first TimeDistributed(QuaternionDense) on
    the (B, C, F, T) body output (interspeech_model.py:140-149) is an (F, 1) 'valid' conj-convolution whose kernel is the dense weight
    with rows (cq, f) instead of (f, cq).  Reading the PARAMETER in place must give exactly what the permuted copy gives -- forward,
    backward-data, and the kernel gradient written straight in the parameter's own layout -- and everything outside the 16-bit
    matrix-core kernels must refuse the order instead of mis-reading it."""
    import qcnn_amd
    from qcnn_amd import _lib
    F = qcnn_amd.functional
    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(21)
    B, Fr, T, cq, units = 3, 14, 37, 64, 256
    x = torch.randn(B, Fr, T, 4 * cq, device=dev, generator=g).to(dtype)
    r = torch.nn.Parameter(torch.randn(cq * Fr, units, device=dev, generator=g) / 40)            # dense weight: row cq_i * Fr + f
    b = torch.nn.Parameter(torch.randn(units, device=dev, generator=g) / 10)
    w_copy = r.detach().view(cq, Fr, units).permute(1, 0, 2).unsqueeze(1).contiguous().requires_grad_(True)   # (Fr, 1, cq, units)
    b2 = b.detach().clone().requires_grad_(True)
    dy = torch.randn(B, 1, T, units, device=dev, generator=g).to(dtype)
    with _lib.debug_flags(_lib.QK_DBG_DETERMINISTIC):          # one addition per gradient element: the two layouts must agree bit for bit
        xa = x.clone().requires_grad_(True)
        ya = F.quaternion_conv_chain(xa, [(r, b, dict(activation='relu', dense_kernel_size=(Fr, 1)))])
        pa = _lib.last_path()
        ya.backward(dy)
        xb = x.clone().requires_grad_(True)
        yb = F.quaternion_conv_chain(xb, [(w_copy, b2, dict(strides=1, padding='valid', dilation_rate=1, activation='relu', conj=True))])
        yb.backward(dy)
        torch.cuda.synchronize()
    assert tuple(ya.shape) == (B, 1, T, units) and torch.equal(ya, yb) and torch.equal(xa.grad, xb.grad)
    assert r.grad.shape == r.shape
    want = w_copy.grad.squeeze(1).permute(1, 0, 2).reshape(r.shape)
    assert torch.equal(r.grad, want) and torch.equal(b.grad, b2.grad) and float(r.grad.abs().max()) > 0
    assert '_qk_prep' in r.__dict__ and len(r._qk_prep) >= 1                         # the parameter carries the cached re-layout
    # fp32 descriptors, channel counts off the matrix-core path: refused, never mis-read
    call = F.conv_call(tuple(x.shape), (Fr, 1, cq, units), torch.float32, 2, 1, 'valid', 'channels_last', 1, None, True, True,
                       kernel_order=_lib.QK_KERNEL_CHANNEL_MAJOR)
    with pytest.raises(RuntimeError, match='kernel_order'):
        call.fwd(x.float(), r.detach(), b.detach())
    call = F.conv_call((B, Fr, T, 4 * 24), (Fr, 1, 24, units), dtype, 2, 1, 'valid', 'channels_last', 1, None, True, True,
                       kernel_order=_lib.QK_KERNEL_CHANNEL_MAJOR)
    with pytest.raises(RuntimeError, match='kernel_order'):
        call.fwd(x[..., :96].contiguous(), r.detach()[:24 * Fr].contiguous(), b.detach())


@pytest.mark.parametrize('cq,fq', [(16, 16), (32, 16)], ids=['16to16', '32to16'])
def test_cached_workspace_of_a_small_channel_layer_serves_both_kernels_in_any_order(cq, fq):
    """Round-5 advisor: a 16 / 32-channel layer's cached 16-bit kernel held ONE of two layouts (k_hconv16_small's fragments or the
    band kernel's), chosen per call, with nothing recording which -- a PReLU forward (band form) followed by a plain forward on the
    same parameter ran the small kernel on band-layout bytes.  Now the workspace carries both layouts in regions of their own
    (qk_conv_workspace_bytes grows by the fragment region; a miss and qk_conv_prep_kernels fill both): every interleaving of the two
    forms on one cached buffer equals the un-cached result bit for bit, and the refresh behind an optimiser step keeps both valid."""
    import qcnn_amd
    from qcnn_amd import _lib
    F = qcnn_amd.functional
    dev = _dev()
    dt = torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(11)
    xs, ws = (3, 7, 90, 4 * cq), (3, 5, cq, 4 * fq)
    x = torch.randn(xs, device=dev, generator=g).to(dt)
    w = torch.nn.Parameter(torch.randn(ws, device=dev, generator=g) / 20)
    b = torch.randn(4 * fq, device=dev, generator=g) / 10
    alpha = torch.full((1,), 0.25, device=dev)
    call = F.conv_call(xs, ws, dt, 2, 1, 'same', 'channels_last', 1, None, True, False)
    band_bytes = 15 * 32 * 4 * 32 * 2 + 256
    assert call._kernel_only_bytes(_lib.QK_OP_FWD) > band_bytes             # the second region exists for this shape

    def plain(cached):
        y = call.fwd(x, w.detach(), b, wparam=w if cached else None)
        return y, _lib.last_path()

    def prelu(cached):
        pre, y = call.fwd_post(x, w.detach(), b, F.PostOp(alpha, -1, 0.0, 0), wparam=w if cached else None)
        return (pre, y), _lib.last_path()
    y_ref, p0 = plain(False)
    (pre_ref, yp_ref), p1 = prelu(False)
    assert (p0, p1) == ('mfma16_small', 'mfma16_band'), (p0, p1)
    for order in ((prelu, plain, prelu, plain), (plain, prelu, plain)):
        w.__dict__.pop('_qk_prep', None)
        for step, fn in enumerate(order):
            out, path = fn(True)
            if fn is plain:
                assert path == 'mfma16_small' and torch.equal(out, y_ref), (step, path)
            else:
                assert path == 'mfma16_band' and torch.equal(out[0], pre_ref) and torch.equal(out[1], yp_ref), (step, path)
        assert len(w._qk_prep) == 1                                          # ONE cached buffer served all of them
    # the batched refresh (behind Adam) rewrites both regions: change the weights through a raw write + refresh, both forms follow
    with torch.no_grad():
        w.mul_(1.5)
    F.refresh_prepped_kernels()
    y2, _ = plain(True)
    (pre2, _y2p), _ = prelu(True)
    y2_ref, _ = plain(False)
    (pre2_ref, _x), _ = prelu(False)
    assert torch.equal(y2, y2_ref) and torch.equal(pre2, pre2_ref) and not torch.equal(y2, y_ref)
    # the diagnostic switch may now be flipped at run time on a cached buffer (the band region is always valid)
    with _lib.debug_flags(_lib.QK_DBG_NO_SMALL16):
        y3, p3 = plain(True)
    assert p3 == 'mfma16_band' and float((y3.float() - y2_ref.float()).abs().max()) <= 1e-2 * float(y2_ref.float().abs().max())


@pytest.mark.parametrize('dtype,tol', [(torch.float32, 1e-4), (torch.bfloat16, 1e-2)], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('fmt', ['channels_first', 'channels_last'])
def test_first_layer_tap_folding_matches_oracle(dtype, tol, fmt):
    """Cq = 1 layers whose input needs no gradient run as a 1x1 conv on the tap-folded input
    (qk_conv_fold_taps); results must equal the oracle's plain convolution."""
    import qcnn_amd
    from oracle import oracle
    F = qcnn_amd.functional
    dev = _dev()
    rng = np.random.RandomState(5)
    xs = (3, 4, 41, 23) if fmt == 'channels_first' else (3, 41, 23, 4)
    x = torch.tensor(rng.randn(*xs).astype(np.float32)).to(dtype).float().numpy()
    w = torch.tensor((rng.randn(3, 5, 1, 64) / 8).astype(np.float32)).to(dtype).float().numpy()
    b = (0.1 * rng.randn(64)).astype(np.float32)
    kw = dict(padding='same', activation='relu', data_format=fmt)
    y = oracle.forward(x, w, b, 2, **kw)
    dy = torch.tensor(rng.randn(*y.shape).astype(np.float32)).to(dtype).float().numpy()
    _, dw, db = oracle.backward(x, w, b, dy, 2, y=y, **kw)
    xt = torch.tensor(x, device=dev).to(dtype)                      # no requires_grad -> folded path
    wt = torch.tensor(w, device=dev, requires_grad=True)
    bt = torch.tensor(b, device=dev, requires_grad=True)
    yt = F.quaternion_conv(xt, wt, bt, **kw)
    yt.backward(torch.tensor(dy, device=dev).to(dtype))
    assert tuple(yt.shape) == y.shape
    assert _rel_err(yt.detach().float().cpu().numpy(), y) <= tol
    assert _rel_err(wt.grad.cpu().numpy(), dw) <= max(tol / 5, 1e-4)
    assert _rel_err(bt.grad.cpu().numpy(), db) <= max(tol / 5, 1e-4)
    y_plain = F.quaternion_conv(xt, wt, bt, fold_small_cq=False, **kw)   # the unfolded kernels agree
    assert _rel_err(y_plain.detach().float().cpu().numpy(), yt.detach().float().cpu().numpy()) <= tol


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'fp16'])
def test_point_form_kernel_serves_one_tap_per_row_shapes(dtype):
    """k_hgemm16_point (streaming form: kernel slice resident in LDS, A fragments straight from global memory) takes
    1 x 1 / dense forwards and the backward-data of a kernel-spans-the-axis 'valid' convolution (the TIMIT head);
    qk_last_path reports it, QK_DBG_NO_POINT16 routes the same call to the implicit-GEMM kernel, and both match the
    oracle (rows not a multiple of the 128-row tile, more units than workgroups so kernel slices get reloaded)."""
    import qcnn_amd
    from qcnn_amd import _lib
    from oracle import oracle
    F = qcnn_amd.functional
    dev = _dev()
    rng = np.random.RandomState(3)
    rnd = lambda *s: torch.tensor(rng.randn(*s).astype(np.float32)).to(dtype).float().numpy()
    tol = 1e-2 if dtype == torch.bfloat16 else 2e-3
    # backward-data of an (F, 1) 'valid' conj convolution: 9 taps x 5 row tiles x 2 column blocks
    xs, ws = (37, 9, 17, 512), (9, 1, 128, 256)
    w = (rnd(*ws) / 30).astype(np.float32)
    w = torch.tensor(w).to(dtype).float().numpy()
    dy = rnd(37, 1, 17, 256)
    call = F.conv_call(xs, ws, dtype, 2, 1, 'valid', 'channels_last', 1, None, True, True)
    wt, dyt = torch.tensor(w, device=dev), torch.tensor(dy, device=dev).to(dtype)
    dx = call.bwd_data(dyt, None, wt)
    assert _lib.last_path() == 'mfma16_point'
    with _lib.debug_flags(_lib.QK_DBG_NO_POINT16):
        dx_gemm = call.bwd_data(dyt, None, wt)
        assert _lib.last_path() == 'mfma16'
    want, _, _ = oracle.backward(np.zeros(xs, np.float32), w, None, dy, 2, padding='valid', activation=None, conj=True)
    assert _rel_err(dx.float().cpu().numpy(), want) <= tol
    assert _rel_err(dx_gemm.float().cpu().numpy(), want) <= tol
    # 1 x 1 forward with bias and relu, 32 -> 128 quaternion channels (two column blocks)
    xs, ws = (5, 61, 128), (1, 32, 512)
    x, w, b = rnd(*xs), torch.tensor((rnd(*ws) / 8)).to(dtype).float().numpy(), (0.1 * rng.randn(512)).astype(np.float32)
    call = F.conv_call(xs, ws, dtype, 1, 1, 'same', 'channels_last', 1, 'relu', True, False)
    y = call.fwd(torch.tensor(x, device=dev).to(dtype), torch.tensor(w, device=dev), torch.tensor(b, device=dev))
    assert _lib.last_path() == 'mfma16_point'
    assert _rel_err(y.float().cpu().numpy(), oracle.forward(x, w, b, 1, padding='same', activation='relu')) <= tol


def test_cpu_tensor_raises_no_fallback():
    import qcnn_amd
    x = torch.randn(2, 10, 8)
    w = torch.randn(3, 2, 8)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        qcnn_amd.functional.quaternion_conv(x, w)


def test_layer_api_on_device_matches_golden():
    """The Keras-style layer objects (build/call) drive the same path."""
    from qcnn_amd.complexnn import QuaternionConv2D, QuaternionDense
    dev = _dev()
    rec, cfg = load_golden([f for f in FILES if 'g06_' in f][0])
    layer = QuaternionConv2D(4, (3, 5), padding='same', data_format='channels_first', activation='relu')
    x = torch.tensor(rec['x'], device=dev)
    layer(x)
    with torch.no_grad():
        layer.kernel.copy_(torch.tensor(rec['kernel'], device=dev))
        layer.bias.copy_(torch.tensor(rec['bias'], device=dev))
    y = layer(x)
    assert tuple(y.shape) == tuple(rec['y'].shape)
    assert _rel_err(y.detach().cpu().numpy(), rec['y']) <= 1e-4
    rec, cfg = load_golden([f for f in FILES if 'g10_' in f][0])
    d = QuaternionDense(12, activation='relu')
    x = torch.tensor(rec['x'], device=dev)
    d(x)
    with torch.no_grad():
        d.r.copy_(torch.tensor(rec['kernel'], device=dev))
        d.bias.copy_(torch.tensor(rec['bias'], device=dev))
    assert _rel_err(d(x).detach().cpu().numpy(), rec['y']) <= 1e-4


FULL_SIZE_SHAPES = [('32to32', 32, 32), ('32to64', 32, 64), ('64to64', 64, 64)]


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('shape', FULL_SIZE_SHAPES, ids=[c[0] for c in FULL_SIZE_SHAPES])
def test_full_size_properties_cfg3_body(shape, dtype):
    """The three body-layer shapes of BASELINE config 3 at the FULL batch (B = 256: the oracle would take hours):
    oracle-independent, size-independent properties --
      * linearity in x (fp32; in 16 bit the rounding of the output is not linear),
      * the adjoint identities  <dy, A x> = <A^T dy, x> = <dW(x, dy), W>  (A = the layer as a linear map of x, and of W)
        with dy CORRELATED with y, so that the common value is of the size ||y||^2 and the comparison is relative to
        it: a kernel that dropped or double-counted even a thousandth of the rows (tile borders, padded band
        positions, the split of M in backward-weight) moves one side by that fraction.  Rounding (fp32 accumulation;
        one 16-bit rounding of y and dx) is unbiased and averages out over 10^8 elements: 1e-5 / 2e-3."""
    import qcnn_amd
    F = qcnn_amd.functional
    dev = _dev()
    _, cq, fq = shape
    g = torch.Generator(device=dev).manual_seed(0)
    B = 256
    x1 = torch.randn(B, 14, 200, 4 * cq, device=dev, generator=g).to(dtype)
    w = (torch.randn(3, 5, cq, 4 * fq, device=dev, generator=g) / np.sqrt(60.0 * cq)).requires_grad_(True)
    kw = dict(padding='same', activation=None)
    if dtype == torch.float32:
        x2 = torch.randn(B, 14, 200, 4 * cq, device=dev, generator=g)
        y1 = F.quaternion_conv(x1, w, None, **kw).detach()
        y2 = F.quaternion_conv(x2, w, None, **kw).detach()
        y12 = F.quaternion_conv(x1 + 2 * x2, w, None, **kw).detach()
        lin = float((y12 - (y1 + 2 * y2)).abs().max() / y12.abs().max())
        assert lin <= 1e-5, 'linearity %.3g' % lin
        del x2, y1, y2, y12
    xa = x1.requires_grad_(True)
    y = F.quaternion_conv(xa, w, None, **kw)
    dy = (y.detach().float() + 0.5 * torch.randn(y.shape, device=dev, generator=g)).to(dtype)
    y.backward(dy)
    assert qcnn_amd._lib.last_path() != 'none'
    dot = lambda a, b: float((a.double() * b.double()).sum())
    lhs = dot(y.detach(), dy)
    rhs_x = dot(xa.grad, xa.detach())
    rhs_w = dot(w.grad, w.detach())
    tol = 1e-5 if dtype == torch.float32 else 2e-3
    assert lhs > 0.5 * float(y.detach().double().norm()) ** 2
    assert abs(lhs - rhs_x) <= tol * lhs, ('adjoint x', lhs, rhs_x, abs(lhs - rhs_x) / lhs)
    assert abs(lhs - rhs_w) <= tol * lhs, ('adjoint w', lhs, rhs_w, abs(lhs - rhs_w) / lhs)


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16], ids=['fp16', 'bf16'])
def test_cfg5_full_stack_homogeneity_identities(dtype):
    """BASELINE configs[4] per GPU at FULL depth and size: QuaternionConv2D 1 -> 256, 9 x (256 -> 256) (3,5) 'same'
    relu, TimeDistributed QuaternionDense(256) head (in_q = 3584), 32 samples of (14, 200), exactly the chain
    bench.StackTrainStep times.  No oracle can run this; but a bias-free relu network is positively homogeneous of
    degree 1 in its input AND in each layer's kernel, so by Euler's theorem
            <dy, y>  =  <dL/dW_l, W_l>   for EVERY layer l   ( =  <dL/dx, x> )
    where dL/d. are the gradients the backward returns for the cotangent dy.  Eleven independent checks of the whole
    backward (every backward-data feeds the layers below it, every backward-weight is one of the identities), with dy
    correlated with y so that the common value is large: a relative tolerance of 1 % covers ten layers of 16-bit rounding
    (observed ~1e-3) and would catch a lost tile, tap, split or sign in any of the 31 kernels."""
    import qcnn_amd
    from qcnn_amd.complexnn.init import qconv_init
    F = qcnn_amd.functional
    dev = _dev()
    B, Fr, T, W, body = 32, 14, 200, 256, 9
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(B, Fr, T, 4, device=dev, generator=g).to(dtype)
    np.random.seed(0)
    shapes = [(3, 5, 1, 4 * W)] + [(3, 5, W, 4 * W)] * body + [(Fr, 1, W, 256)]
    ws = []
    for s_ in shapes:
        w0 = qconv_init(kernel_size=s_[:2], input_dim=s_[2], weight_dim=2, nb_filters=s_[3] // 4, criterion='he')()
        ws.append(torch.nn.Parameter(torch.tensor(w0, dtype=torch.float32, device=dev)))
    kws = [dict(padding='same', activation='relu')] * (1 + body) + [dict(padding='valid', activation='relu', conj=True)]
    h = F.quaternion_conv(x, ws[0], None, **kws[0])
    y = F.quaternion_conv_chain(h, [(ws[i], None, kws[i]) for i in range(1, len(ws))])
    assert float((y.detach() > 0).float().mean()) > 0.05                 # the network is alive down to the head
    dy = (y.detach().float() * (1.0 + 0.5 * torch.randn(y.shape, device=dev, generator=g))).to(dtype)
    y.backward(dy)
    dot = lambda a, b: float((a.double() * b.double()).sum())
    lhs = dot(y.detach(), dy)
    assert lhs > 0
    errs = [abs(dot(w_.grad, w_.detach()) - lhs) / lhs for w_ in ws]
    assert max(errs) <= 1e-2, errs


FULL_SIZE_16BIT = [
    # BASELINE config 3, stage-2 body layer at the full batch (the Hamilton GEMM of the 40 % target)
    ('cfg3_body_b256_bf16', torch.bfloat16, (256, 14, 200, 256), (3, 5, 64, 256)),
    # config 3 stage-1 body layer (32 -> 32 filters) and the 32 -> 64 transition, full batch
    ('cfg3_stage1_b256_bf16', torch.bfloat16, (256, 14, 200, 128), (3, 5, 32, 128)),
    ('cfg3_32to64_b256_bf16', torch.bfloat16, (256, 14, 200, 128), (3, 5, 32, 256)),
    # config 5 body layer (Cq = F = 256, fp16), 32 samples per GPU
    ('cfg5_body_b32_fp16', torch.float16, (32, 14, 200, 1024), (3, 5, 256, 1024)),
    # config 3 head: TimeDistributed(QuaternionDense(256)) on B*T = 51 200 rows of 3584 features
    ('cfg3_head_dense_bf16', torch.bfloat16, (51200, 3584), (896, 256)),
]


@pytest.mark.parametrize('case', FULL_SIZE_16BIT, ids=[c[0] for c in FULL_SIZE_16BIT])
def test_full_size_16bit_mfma_kernels_agree_with_exact_fp32_kernels(case):
    """At BASELINE's full sizes the oracle would run for hours, so the 16-bit MFMA kernels (k_hgemm16,
    k_wgrad16) are checked against the general fp32-MFMA kernels on the SAME 16-bit inputs: those are an
    exact fp32 fmaf chain and are themselves pinned to the oracle above at every small shape.  Both see
    identical operands (the fp32 kernel also rounds its output to 16 bits), so the only differences are
    the kernel rounded to 16 bits for the matrix cores and the accumulation order.  QK_DBG_NO_MFMA16 is the
    library's diagnostic switch (qk_set_debug_flags)."""
    import qcnn_amd
    F = qcnn_amd.functional
    _, dtype, xs, ws = case
    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(21)
    x = torch.randn(xs, device=dev, generator=g).to(dtype)
    # kernel values exactly representable in 16 bits: both paths then multiply identical numbers
    w = (torch.randn(ws, device=dev, generator=g) / (4.0 * (ws[-2] * (15 if len(ws) > 2 else 1)) ** 0.5)).to(dtype).float()
    b = (torch.randn(ws[-1], device=dev, generator=g) / 10).to(dtype).float()
    if len(xs) == 2:
        call = F.dense_call(tuple(xs), tuple(ws), dtype, 'relu', True)
    else:
        call = F.conv_call(tuple(xs), tuple(ws), dtype, 2, 1, 'same', 'channels_last', 1, 'relu', True)

    dy = torch.randn(call.y_shape, device=dev, generator=g).to(dtype)

    def run(y_mask):
        y = call.fwd(x, w, b)
        # the same relu mask for both paths: an element of y that rounds to 0 on one path and to a tiny
        # positive number on the other would otherwise switch a whole dy element on or off
        dx, dw, db = call.bwd(x, dy, y if y_mask is None else y_mask, w, True)
        torch.cuda.synchronize()
        return y, dx, dw, db

    from qcnn_amd import _lib
    fast = run(None)
    assert _lib.last_path() in ('mfma16', 'mfma16_band', 'mfma16_point')
    with _lib.debug_flags(_lib.QK_DBG_NO_MFMA16):
        exact = run(fast[0])
        assert _lib.last_path() == 'fp32_mfma'
    assert not torch.equal(fast[2], exact[2]), 'QK_DBG_NO_MFMA16 did not switch kernels: the check is vacuous'
    # y: identical up to the last 16-bit rounding (and relu flips of values that round across zero)
    tol16 = 1e-2 if dtype == torch.bfloat16 else 2e-3
    names = ('y', 'dx', 'dkernel', 'dbias')
    for name, a, e in zip(names, fast, exact):
        a, e = a.float(), e.float()
        err = float((a - e).abs().max()) / float(e.abs().max())
        tol = tol16 if name in ('y', 'dx') else 2e-3
        assert err <= tol, '%s: rel err %.3g > %.1g' % (name, err, tol)
        # and no systematic drift: the sums agree much more tightly than single elements
        ssum = abs(float(a.double().sum()) - float(e.double().sum())) / float(e.double().abs().sum())
        assert ssum <= 1e-4, '%s: checksum drift %.3g' % (name, ssum)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'fp16'])
def test_full_size_head_convolution_backward_agrees_with_exact_fp32_kernels(dtype):
    """The TimeDistributed head of the B = 256 model as the (14, 1) 'valid' conj convolution the chain runs, with the
    chain's QK_BWD_MASK_DX flag: forward (k_hgemm16, 14 taps), backward-weight (k_wgrad16) and the backward-data in its
    streaming point form with the epilogue mask (k_hgemm16_point), against the exact fp32-MFMA kernels on the same
    16-bit operands."""
    import qcnn_amd
    from qcnn_amd import _lib
    F = qcnn_amd.functional
    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(77)
    xs, ws = (256, 14, 200, 256), (14, 1, 64, 256)
    x = torch.relu(torch.randn(xs, device=dev, generator=g)).to(dtype)           # a relu layer's output (it is also the mask)
    w = (torch.randn(ws, device=dev, generator=g) / (4.0 * (64 * 14) ** 0.5)).to(dtype).float()
    b = (torch.randn(256, device=dev, generator=g) / 10).to(dtype).float()
    call = F.conv_call(xs, ws, dtype, 2, 1, 'valid', 'channels_last', 1, 'relu', True, True)
    dy = torch.randn(call.y_shape, device=dev, generator=g).to(dtype)

    def run(y_mask):
        y = call.fwd(x, w, b)
        dx, dw, db = call.bwd(x, dy, y if y_mask is None else y_mask, w, True, flags=_lib.QK_BWD_MASK_DX)
        torch.cuda.synchronize()
        return y, dx, dw, db

    fast = run(None)
    assert _lib.last_path() == 'mfma16_point'
    with _lib.debug_flags(_lib.QK_DBG_NO_MFMA16):
        exact = run(fast[0])
        assert _lib.last_path() == 'fp32_mfma'
    assert float((fast[1].float() * (x.float() <= 0)).abs().max()) == 0.0          # the mask is applied
    tol16 = 1e-2 if dtype == torch.bfloat16 else 2e-3
    for name, a, e in zip(('y', 'dx', 'dkernel', 'dbias'), fast, exact):
        a, e = a.float(), e.float()
        err = float((a - e).abs().max()) / float(e.abs().max())
        assert err <= (tol16 if name in ('y', 'dx') else 2e-3), '%s: rel err %.3g' % (name, err)
        ssum = abs(float(a.double().sum()) - float(e.double().sum())) / float(e.double().abs().sum())
        assert ssum <= 1e-4, '%s: checksum drift %.3g' % (name, ssum)


def test_masked_dy_side_output_and_fused_backward_agree():
    """bwd_weight can leave dy*(y>0) for bwd_data (the DP step's ordering); the fused qk_conv_bwd and the
    two-call sequence must give the same gradients as the separate masked calls."""
    import qcnn_amd
    F = qcnn_amd.functional
    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(3)
    for dtype in (torch.float32, torch.bfloat16):
        x = torch.randn(3, 40, 128, device=dev, generator=g).to(dtype)
        w = torch.randn(3, 32, 128, device=dev, generator=g) / 20
        b = torch.randn(128, device=dev, generator=g) / 10
        call = F.conv_call(tuple(x.shape), tuple(w.shape), dtype, 1, 1, 'same', 'channels_last', 1, 'relu', True)
        lin = F.conv_call(tuple(x.shape), tuple(w.shape), dtype, 1, 1, 'same', 'channels_last', 1, 'linear', True)
        y = call.fwd(x, w, b)
        dy = torch.randn(y.shape, device=dev, generator=g).to(dtype)
        dx_ref = call.bwd_data(dy, y, w)
        dw_ref, db_ref = call.bwd_weight(x, dy, y, True)
        dym = torch.empty((dy.numel() + 127) // 128 * 128, dtype=dtype, device=dev)
        dw2, db2 = call.bwd_weight(x, dy, y, True, masked_dy_out=dym)
        want = torch.where(y > 0, dy, torch.zeros_like(dy))
        assert torch.equal(dym[:dy.numel()].view_as(dy), want)
        dx2 = lin.bwd_data(dym[:dy.numel()].view_as(dy), None, w)
        dx3, dw3, db3 = call.bwd(x, dy, y, w, True)
        tol = 1e-5 if dtype == torch.float32 else 1e-2
        for got, ref in ((dx2, dx_ref), (dx3, dx_ref), (dw2, dw_ref), (dw3, dw_ref), (db2, db_ref), (db3, db_ref)):
            assert _rel_err(got.float().cpu().numpy(), ref.float().cpu().numpy()) <= tol


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'fp16'])
@pytest.mark.parametrize('xs,ws', [((2, 14, 40, 128), (3, 5, 32, 128)), ((1, 14, 40, 256), (3, 5, 64, 256)),
                                   ((1, 9, 33, 128), (3, 3, 32, 256)), ((3, 70, 256), (5, 64, 128))],
                         ids=['32to32', '64to64', '32to64', 'conv1d_64to32'])
def test_masked_dy_side_output_is_bit_exact_and_repeatable(xs, ws, dtype):
    """dy * (y > 0) is a pure selection, so the side output of the 16-bit backward-weight kernel must
    equal torch.where bit for bit on every run (a store-data hazard once corrupted a few lanes of it,
    non-deterministically; gradients themselves were unaffected)."""
    import qcnn_amd
    F = qcnn_amd.functional
    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(3)
    rank = len(xs) - 2
    x = torch.randn(xs, device=dev, generator=g).to(dtype)
    w = torch.randn(ws, device=dev, generator=g) / 20
    b = torch.randn(ws[-1], device=dev, generator=g) / 10
    call = F.conv_call(tuple(xs), tuple(ws), dtype, rank, 1, 'same', 'channels_last', 1, 'relu', True)
    y = call.fwd(x, w, b)
    dy = torch.randn(y.shape, device=dev, generator=g).to(dtype)
    want = torch.where(y > 0, dy, torch.zeros_like(dy))
    dw0 = None
    for rep in range(10):
        dym = torch.full(((dy.numel() + 127) // 128 * 128,), 7.0, dtype=dtype, device=dev)
        dw, db = call.bwd_weight(x, dy, y, True, masked_dy_out=dym)
        assert torch.equal(dym[:dy.numel()].view_as(dy), want), 'run %d' % rep
        assert bool((dym[dy.numel():] == 7.0).all()), 'wrote past the end of dy'
        if dw0 is None:
            dw0 = dw.clone()
        assert _rel_err(dw.cpu().numpy(), dw0.cpu().numpy()) <= 1e-5      # atomics: order varies, values barely


def test_adam_step_matches_keras_formula():
    import qcnn_amd
    dev = _dev()
    rng = np.random.RandomState(0)
    n = 10007
    p, g = rng.randn(n).astype(np.float32), rng.randn(n).astype(np.float32)
    m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    tp, tg = torch.tensor(p, device=dev), torch.tensor(g, device=dev)
    tm, tv = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    lr, b1, b2, eps = 5e-4, 0.9, 0.999, 1e-7
    p64, m64, v64 = p.astype(np.float64), m.astype(np.float64), v.astype(np.float64)
    for t in (1, 2, 3):
        qcnn_amd.functional.adam_step(tp, tg, tm, tv, t, lr=lr, beta1=b1, beta2=b2, eps=eps, grad_scale=0.5)
        gs = 0.5 * g.astype(np.float64)
        m64 = b1 * m64 + (1 - b1) * gs
        v64 = b2 * v64 + (1 - b2) * gs * gs
        p64 = p64 - lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t) * m64 / (np.sqrt(v64) + eps)
    assert np.abs(tp.cpu().numpy() - p64).max() <= 1e-5
    assert np.abs(tm.cpu().numpy() - m64).max() <= 1e-6


def test_empty_batch_gives_empty_output_and_zero_gradients():
    import qcnn_amd
    F = qcnn_amd.functional
    dev = _dev()
    for dtype in (torch.float32, torch.bfloat16):
        x = torch.zeros(0, 9, 11, 8, device=dev, dtype=dtype, requires_grad=True)
        w = torch.randn(3, 2, 2, 12, device=dev, requires_grad=True)
        b = torch.zeros(12, device=dev, requires_grad=True)
        y = F.quaternion_conv(x, w, b, padding='same', strides=(2, 1), activation='relu')
        assert tuple(y.shape) == (0, 5, 11, 12) and y.dtype == dtype
        y.sum().backward()
        assert float(w.grad.abs().max()) == 0.0 and float(b.grad.abs().max()) == 0.0 and x.grad.shape == x.shape
        yc = F.quaternion_conv(x.detach().permute(0, 3, 1, 2), w.detach(), None, padding='valid',
                               data_format='channels_first')
        assert tuple(yc.shape) == (0, 12, 7, 10)
        xd = torch.zeros(0, 16, device=dev, dtype=dtype)
        assert tuple(F.quaternion_dense(xd, torch.randn(4, 8, device=dev), None).shape) == (0, 8)


RAGGED_CASES = [
    # rows that do not fill a tile, a kernel wider than the input, single-position outputs, one sample
    ('one_row', 1, (1, 1, 8), (3, 2, 8), dict(padding='same', activation='relu')),
    ('kernel_wider_than_input', 1, (2, 3, 16), (7, 4, 8), dict(padding='same', activation=None)),
    ('valid_to_single_position', 2, (3, 3, 5, 8), (3, 5, 2, 16), dict(padding='valid', activation='relu')),
    ('m_not_multiple_of_tile', 1, (3, 43, 128), (3, 32, 128), dict(padding='same', activation='relu')),
    ('causal_dilated', 1, (2, 37, 16), (4, 4, 8), dict(padding='causal', dilation_rate=3, activation='relu')),
    ('dense_one_row', 0, (1, 128), (32, 128), dict(activation='relu')),
]


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('case', RAGGED_CASES, ids=[c[0] for c in RAGGED_CASES])
def test_ragged_and_degenerate_shapes_match_oracle(case, dtype):
    import qcnn_amd
    _, rank, xs, ws, kw = case
    x, w, b, dy, want = _oracle_case(rank, xs, ws, kw, seed=5, dtype=dtype)
    got = _run_layer(qcnn_amd.functional, x, w, b, dy, rank, kw, dtype)
    tol16, tol32 = (1e-4, 1e-4) if dtype == torch.float32 else (1e-2, 2e-3)
    for k, v in got.items():
        err = _rel_err(v, want[k])
        assert err <= (tol16 if k in ('y', 'dx') else tol32), '%s: rel err %.3g' % (k, err)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_accumulating_backward_weight_and_zeroing_adam(dtype):
    """qk_*_bwd_weight_acc adds into dw / dbias; qk_adam_step_zero_grad == qk_adam_step + cleared gradient."""
    import qcnn_amd
    F = qcnn_amd.functional
    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(8)
    x = torch.randn(4, 40, 128, device=dev, generator=g).to(dtype)
    w = torch.randn(3, 32, 128, device=dev, generator=g) / 20
    b = torch.randn(128, device=dev, generator=g) / 10
    call = F.conv_call(tuple(x.shape), tuple(w.shape), dtype, 1, 1, 'same', 'channels_last', 1, 'relu', True)
    y = call.fwd(x, w, b)
    dy = torch.randn(y.shape, device=dev, generator=g).to(dtype)
    dw, db = call.bwd_weight(x, dy, y, True)
    acc_w, acc_b = torch.full_like(dw, 0.5), torch.full_like(db, -0.25)
    call.bwd_weight(x, dy, y, True, out=(acc_w, acc_b), accumulate=True)
    call.bwd_weight(x, dy, y, True, out=(acc_w, acc_b), accumulate=True)
    assert _rel_err((acc_w - 0.5).cpu().numpy(), (2 * dw).cpu().numpy()) <= 1e-5
    assert _rel_err((acc_b + 0.25).cpu().numpy(), (2 * db).cpu().numpy()) <= 1e-5
    xd = torch.randn(50, 128, device=dev, generator=g).to(dtype)
    wd = torch.randn(32, 64, device=dev, generator=g) / 10
    dcall = F.dense_call(tuple(xd.shape), tuple(wd.shape), dtype, 'linear', False)
    dyd = torch.randn(50, 64, device=dev, generator=g).to(dtype)
    dwd, _ = dcall.bwd_weight(xd, dyd, None, False)
    accd = torch.ones_like(dwd)
    dcall.bwd_weight(xd, dyd, None, False, out=(accd, None), accumulate=True)
    assert _rel_err((accd - 1).cpu().numpy(), dwd.cpu().numpy()) <= 1e-5
    # Adam
    n = 1000
    p1 = torch.randn(n, device=dev, generator=g); p2 = p1.clone()
    gr = torch.randn(n, device=dev, generator=g); gr2 = gr.clone()
    m1 = torch.zeros(n, device=dev); v1 = torch.zeros(n, device=dev); m2 = m1.clone(); v2 = v1.clone()
    F.adam_step(p1, gr, m1, v1, 3, lr=1e-3, grad_scale=0.5)
    F.adam_step(p2, gr2, m2, v2, 3, lr=1e-3, grad_scale=0.5, zero_grad=True)
    assert torch.equal(p1, p2) and torch.equal(m1, m2) and torch.equal(v1, v2)
    assert float(gr2.abs().max()) == 0.0 and float(gr.abs().max()) > 0.0


def test_c_abi_reports_errors_instead_of_faulting():
    import ctypes
    import qcnn_amd
    from qcnn_amd import _lib
    F = qcnn_amd.functional
    dev = _dev()
    x = torch.randn(2, 16, 128, device=dev).to(torch.bfloat16)
    w = torch.randn(3, 32, 128, device=dev)
    call = F.conv_call(tuple(x.shape), tuple(w.shape), torch.bfloat16, 1, 1, 'same', 'channels_last', 1, 'relu', False)
    y = call.fwd(x, w, None)
    lib = _lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    dx = torch.empty_like(x)
    dw = torch.empty_like(w)
    # fused backward without a workspace
    rc = lib.qk_conv_bwd(ctypes.byref(call.desc), p(x), p(y), p(y), p(w), p(dx), p(dw), None, None, 0, None)
    assert rc == -3 and b'workspace' in lib.qk_last_error()
    # relu backward-data without the forward output
    rc = lib.qk_conv_bwd_data(ctypes.byref(call.desc), p(y), None, p(w), p(dx), None, 0, None)
    assert rc == -1 and b'forward output' in lib.qk_last_error()
    # tap folding with a bad channel count
    rc = lib.qk_conv_fold_taps(ctypes.byref(call.desc), p(x), p(dx), 20, None)
    assert rc == -1 and b'cq2' in lib.qk_last_error()


# ---- round 2: paths that had only met other HIP kernels so far -----------------------------------------------
CONJ_CASES = [
    # conj = 1 convolutions (the dense table, dense.py:139-143, at rank > 0): how the TIMIT head runs
    ('conj_conv1d', 1, (3, 50, 32), (3, 8, 48), dict(padding='same', activation='relu', conj=True)),
    ('conj_conv2d_body', 2, (2, 14, 40, 128), (3, 5, 32, 128), dict(padding='same', activation='relu', conj=True)),
    # the TimeDistributed dense head as an (F, 1) 'valid' convolution over (F, T): every dx row has ONE valid tap
    # (the tile-level tap skip of k_hgemm16), 150 rows per image row -> tiles straddle two taps
    ('conj_head_as_conv', 2, (3, 14, 50, 256), (14, 1, 64, 256), dict(padding='valid', activation='relu', conj=True)),
    ('head_as_conv_linear', 2, (2, 6, 70, 128), (6, 1, 32, 128), dict(padding='valid', activation=None, conj=True)),
    # 'same' padding with a tall kernel: border tiles skip the taps that fall outside for all their rows
    ('tall_kernel_same', 2, (1, 9, 140, 128), (5, 1, 32, 128), dict(padding='same', activation='relu')),
]


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16], ids=['fp32', 'bf16', 'fp16'])
@pytest.mark.parametrize('case', CONJ_CASES, ids=[c[0] for c in CONJ_CASES])
def test_conj_and_tap_skipping_convolutions_match_oracle(case, dtype):
    import qcnn_amd
    _, rank, xs, ws, kw = case
    x, w, b, dy, want = _oracle_case(rank, xs, ws, kw, seed=17, dtype=dtype)
    got = _run_layer(qcnn_amd.functional, x, w, b, dy, rank, kw, dtype)
    tol16, tol32 = {torch.float32: (1e-4, 1e-4), torch.bfloat16: (1e-2, 2e-3), torch.float16: (2e-3, 1e-3)}[dtype]
    if dtype == torch.float32 and kw.get('activation') == 'relu':
        from oracle import oracle
        dx, dw, db = oracle.backward(x, w, b, dy, rank, y=got['y'].astype(np.float64), **kw)
        want = dict(want, dx=dx, dkernel=dw, dbias=db)
    for k, v in got.items():
        err = _rel_err(v, want[k])
        assert err <= (tol16 if k in ('y', 'dx') else tol32), '%s: rel err %.3g' % (k, err)


NATIVE_16BIT = [c for c in ORACLE_CASES if c[0] in ('conv2d_chfirst_body_small', 'conv2d_first_layer')] + [
    ('conv1d_chfirst_native', 1, (3, 32, 45), (3, 8, 64), dict(padding='same', activation='relu', data_format='channels_first')),
    ('conv2d_chfirst_valid_native', 2, (2, 128, 9, 21), (3, 3, 32, 64), dict(padding='valid', activation=None, data_format='channels_first')),
    # Cq, F multiples of 32: the matrix-core path through the workspace re-layout (odd extents: scalar edges of the tiles)
    ('conv2d_chfirst_mfma_same_relu', 2, (2, 128, 7, 23), (3, 5, 32, 128), dict(padding='same', activation='relu', data_format='channels_first')),
    ('conv2d_chfirst_mfma_64_linear', 2, (3, 256, 6, 40), (3, 5, 64, 256), dict(padding='same', activation=None, data_format='channels_first')),
    ('conv1d_chfirst_mfma_valid', 1, (2, 128, 50), (3, 32, 128), dict(padding='valid', activation='relu', data_format='channels_first')),
]


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'fp16'])
@pytest.mark.parametrize('case', NATIVE_16BIT, ids=[c[0] for c in NATIVE_16BIT])
def test_half_native_channels_first_layout_matches_oracle(case, dtype):
    """internal_layout='native' (C-ABI QK_CH_FIRST): true NCHW 16-bit buffers.  Channel counts that are multiples of 32
    run on the 16-bit matrix-core kernels through a re-layout of the operands in the caller's workspace
    (qk_api.hip: cf16_ok; round 2 dropped every such descriptor to the fp32-MFMA kernels, ~10x slower); the others go
    through the generic staging path of the fp32-MFMA kernels (inputs widened while staged, 16-bit outputs)."""
    import qcnn_amd
    _, rank, xs, ws, kw = case
    x, w, b, dy, want = _oracle_case(rank, xs, ws, kw, seed=19, dtype=dtype)
    got = _run_layer(qcnn_amd.functional, x, w, b, dy, rank, dict(kw, fold_small_cq=False), dtype, internal_layout='native')
    on_matrix_cores = ws[-2] % 32 == 0 and ws[-1] % 128 == 0
    assert (qcnn_amd._lib.last_path() != 'fp32_mfma') == on_matrix_cores, qcnn_amd._lib.last_path()
    tol16, tol32 = (1e-2, 2e-3) if dtype == torch.bfloat16 else (2e-3, 1e-3)
    for k, v in got.items():
        err = _rel_err(v, want[k])
        assert err <= (tol16 if k in ('y', 'dx') else tol32), '%s: rel err %.3g' % (k, err)


def _dispatch_cases():
    """(id, rank, x_shape, w_shape, kwargs, native): HALF_CASES and RAGGED_CASES on physically channels_last buffers, NATIVE_16BIT
    on true channels_first ones."""
    out = []
    for group, cases, native in (('half', HALF_CASES, False), ('ragged', RAGGED_CASES, False), ('native', NATIVE_16BIT, True)):
        out += [('%s/%s' % (group, c[0]),) + tuple(c[1:]) + (native,) for c in cases]
    return out


def _dispatch_paths(case):
    """qk_last_path() behind the forward, the backward-data and the backward-weight call of one case, in bf16."""
    import qcnn_amd
    from qcnn_amd import _lib
    F = qcnn_amd.functional
    dev = _dev()
    _, rank, xs, ws, kw, native = case
    dtype = torch.bfloat16
    if rank == 0:
        call = F.dense_call(tuple(xs), tuple(ws), dtype, kw.get('activation'), True)
    else:
        layout = kw.get('data_format', 'channels_last')
        if layout == 'channels_first' and not native:
            xs, layout = (xs[0],) + tuple(xs[2:]) + (xs[1],), 'channels_last'
        call = F.conv_call(tuple(xs), tuple(ws), dtype, rank, kw.get('strides', 1), kw.get('padding', 'valid'), layout,
                           kw.get('dilation_rate', 1), kw.get('activation'), True, kw.get('conj', False))
    g = torch.Generator(device=dev).manual_seed(23)
    x = torch.randn(xs, device=dev, generator=g).to(dtype)
    w = torch.randn(ws, device=dev, generator=g) / 20
    b = torch.randn(ws[-1], device=dev, generator=g) / 10
    paths = []
    y = call.fwd(x, w, b)
    paths.append(_lib.last_path())
    dy = torch.randn(y.shape, device=dev, generator=g).to(dtype)
    call.bwd_data(dy, y if call.relu else None, w)
    paths.append(_lib.last_path())
    call.bwd_weight(x, dy, y if call.relu else None, True)
    paths.append(_lib.last_path())
    torch.cuda.synchronize()
    return paths


def test_every_small_case_is_served_by_the_kernel_family_recorded_for_it():
    """A parity test still passes when a shape silently drops to a slower kernel family, so the dispatch itself is pinned:
    qk_last_path() behind call.fwd, call.bwd_data and call.bwd_weight of every HALF_CASES, RAGGED_CASES and NATIVE_16BIT case in
    bf16 -- the smallest shapes that reach the band, point, small-channel and general 16-bit kernels and the fp32-MFMA fallback --
    against tests/golden/g18_dispatcher.json ('dispatch_paths': id -> [fwd, bwd_data, bwd_weight]), recorded with _dispatch_paths
    on an MI355X from the build of the commit before the dispatcher's geometry and workspace layout got one source each."""
    import json
    from conftest import GOLDEN
    with open(os.path.join(GOLDEN, 'g18_dispatcher.json')) as f:
        want = json.load(f)['dispatch_paths']
    cases = _dispatch_cases()
    assert sorted(want) == sorted(c[0] for c in cases)
    got = {c[0]: _dispatch_paths(c) for c in cases}
    wrong = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not wrong, wrong
    assert {p for v in got.values() for p in v} >= {'mfma16_band', 'mfma16_point', 'mfma16_small', 'mfma16', 'fp32_mfma'}


@pytest.mark.parametrize('form', ['relu_dropout', 'prelu_dropout'])
def test_channels_first_descriptor_with_post_ops_equals_channels_last(form):
    """QK_CH_FIRST at the C-ABI with a post-op (round 2: QK_ERR_UNSUPPORTED): qk_conv_fwd_post / qk_conv_bwd_post on true
    NCHW bf16 buffers against the same calls on the channels-last copies of the same tensors.  The forward runs the same
    kernels on the same values (the dropout mask is a function of the element's index in the channels-last image):
    bit-identical; the gradients agree up to the order of the atomic accumulation."""
    import qcnn_amd
    from qcnn_amd import _lib
    F = qcnn_amd.functional
    dev = _dev()
    dt = torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(3)
    n, cq, fq, h, wd = 2, 32, 64, 6, 40
    x_cl = torch.randn(n, h, wd, 4 * cq, device=dev, generator=g).to(dt)
    dy_cl = torch.randn(n, h, wd, 4 * fq, device=dev, generator=g).to(dt)
    w = torch.randn(3, 5, cq, 4 * fq, device=dev, generator=g) / 30
    b = torch.randn(4 * fq, device=dev, generator=g) / 10
    alpha = (0.05 + 0.3 * torch.rand(h, device=dev, generator=g)) if form == 'prelu_dropout' else None
    post_y = F.PostOp(alpha, 0 if alpha is not None else -1, 0.25, 77)
    alpha_x = (0.05 + 0.3 * torch.rand(h, device=dev, generator=g)) if form == 'prelu_dropout' else None
    post_x = F.PostOp(alpha_x, 0 if alpha_x is not None else -1, 0.25, 78)
    out = {}
    for lay in ('channels_last', 'channels_first'):
        to = (lambda t: t) if lay == 'channels_last' else (lambda t: t.permute(0, 3, 1, 2).contiguous())
        back = (lambda t: t) if lay == 'channels_last' else (lambda t: t.permute(0, 2, 3, 1))
        x, dy = to(x_cl), to(dy_cl)
        call = F.conv_call(tuple(x.shape), tuple(w.shape), dt, 2, 1, 'same', lay, 1, None, True, False)
        pre, y = call.fwd_post(x, w, b, post_y)
        path_f = _lib.last_path()
        # backward of the same layer, its input taken as the output of another post-op (x = post_x(x_pre))
        x_pre = to(torch.randn(n, h, wd, 4 * cq, device=dev, generator=torch.Generator(device=dev).manual_seed(9)).to(dt))
        xin = F.postop_fwd(back(x_pre).contiguous(), post_x)
        xin = to(xin)
        da = torch.zeros(h, device=dev) if alpha_x is not None else None
        dx, dw, db = call.bwd_post(xin, dy, w, True, post_x, x_pre if alpha_x is not None else None, da)
        out[lay] = (back(y), None if pre is None else back(pre), back(dx), dw, db, da, path_f, _lib.last_path())
    a, c = out['channels_last'], out['channels_first']
    assert c[6] != 'fp32_mfma' and c[7] != 'fp32_mfma' and a[6] == c[6]
    assert torch.equal(a[0], c[0]) and (a[1] is None or torch.equal(a[1], c[1]))
    assert torch.equal(a[2], c[2])                                   # backward-data: no atomics in its path
    rel = lambda p, q: float((p - q).abs().max() / q.abs().max())
    assert rel(c[3], a[3]) <= 1e-5 and rel(c[4], a[4]) <= 1e-5
    if a[5] is not None:
        assert rel(c[5], a[5]) <= 1e-4


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_conv_chain_flags_match_oracle_composition(dtype):
    """functional.quaternion_conv_chain (QK_BWD_MASK_DX / QK_BWD_DY_PREMASKED) against the oracle applied layer by
    layer: relu -> relu -> conj 'valid' relu head -- values, input gradient and every kernel / bias gradient.
    16-bit: the composition rounds each layer output to the storage type (forward); backward tolerance covers
    the un-emulated roundings of the intermediate gradients."""
    import qcnn_amd
    from oracle import oracle
    F = qcnn_amd.functional
    dev = _dev()
    rng = np.random.RandomState(23)
    rnd = (lambda a: a) if dtype == torch.float32 else (lambda a: torch.tensor(a).to(dtype).double().numpy())
    specs = [((3, 5, 32, 128), dict(padding='same', activation='relu')),
             ((3, 5, 32, 256), dict(padding='same', activation='relu')),
             ((6, 1, 64, 128), dict(padding='valid', activation='relu', conj=True))]
    x = rnd(rng.randn(2, 6, 40, 128).astype(np.float32).astype(np.float64))
    ws = [rnd((rng.randn(*s) / np.sqrt(np.prod(s[:-1]) * 4)).astype(np.float32).astype(np.float64)) for s, _ in specs]
    bs = [(0.1 * rng.randn(s[-1])).astype(np.float32).astype(np.float64) for s, _ in specs]
    acts = [x]
    for w, b, (_, kw) in zip(ws, bs, specs):
        acts.append(rnd(oracle.forward(acts[-1], w, b, 2, **kw)))
    dy = rnd(rng.randn(*acts[-1].shape).astype(np.float32).astype(np.float64))
    xt = torch.tensor(x, device=dev).to(dtype).requires_grad_(True)
    wt = [torch.tensor(w, device=dev, dtype=torch.float32, requires_grad=True) for w in ws]
    bt = [torch.tensor(b, device=dev, dtype=torch.float32, requires_grad=True) for b in bs]
    y = F.quaternion_conv_chain(xt, [(w, b, kw) for w, b, (_, kw) in zip(wt, bt, specs)])
    y.backward(torch.tensor(dy, device=dev).to(dtype))
    tol_y, tol_g = (1e-4, 1e-4) if dtype == torch.float32 else (1e-2, 3e-2)
    assert _rel_err(y.detach().float().cpu().numpy(), acts[-1]) <= tol_y
    # the backward is compared on the GPU's own activations (relu masks: outputs that are zero up to rounding land
    # on either side of 0): the same kernels layer by layer give the chain's intermediate tensors bit for bit
    acts = [x]
    with torch.no_grad():
        h = xt.detach()
        for w, b, (_, kw) in zip(wt, bt, specs):
            h = F.quaternion_conv(h, w, b, **kw)
            acts.append(h.double().cpu().numpy())
    assert np.array_equal(acts[-1], y.detach().double().cpu().numpy())
    g = dy
    for i in reversed(range(3)):
        g, dw, db = oracle.backward(acts[i], ws[i], bs[i], g, 2, y=acts[i + 1], **specs[i][1])
        assert _rel_err(wt[i].grad.cpu().numpy(), dw) <= tol_g, 'dkernel %d' % i
        assert _rel_err(bt[i].grad.cpu().numpy(), db) <= tol_g, 'dbias %d' % i
    assert _rel_err(xt.grad.float().cpu().numpy(), g) <= tol_g


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('ws', [(7, 7, 1, 32), (5, 5, 2, 64), (3, 7, 2, 32)], ids=['7x7_cq1', '5x5_cq2', '3x7_cq2'])
def test_tap_folding_with_more_than_32_folded_channels(ws, dtype):
    """32 < taps*cq <= 64: the 16-bit fold needs cq2 = 64 (it used to pass 32 and fail with QK_ERR_INVALID_ARG)."""
    import qcnn_amd
    from oracle import oracle
    F = qcnn_amd.functional
    dev = _dev()
    rng = np.random.RandomState(29)
    rnd = lambda a: torch.tensor(a).to(dtype).float().numpy()
    cq = ws[2]
    x = rnd(rng.randn(2, 19, 23, 4 * cq).astype(np.float32))
    w = rnd((rng.randn(*ws) / np.sqrt(np.prod(ws[:-1]) * 4)).astype(np.float32))
    b = (0.1 * rng.randn(ws[-1])).astype(np.float32)
    kw = dict(padding='same', activation='relu')
    y = oracle.forward(x, w, b, 2, **kw)
    dy = rnd(rng.randn(*y.shape).astype(np.float32))
    _, dw, db = oracle.backward(x, w, b, dy, 2, y=y, **kw)
    xt = torch.tensor(x, device=dev).to(dtype)
    wt = torch.tensor(w, device=dev, requires_grad=True)
    bt = torch.tensor(b, device=dev, requires_grad=True)
    yt = F.quaternion_conv(xt, wt, bt, **kw)
    yt.backward(torch.tensor(dy, device=dev).to(dtype))
    tol = 1e-4 if dtype == torch.float32 else 1e-2
    assert _rel_err(yt.detach().float().cpu().numpy(), y) <= tol
    assert _rel_err(wt.grad.cpu().numpy(), dw) <= max(tol / 5, 1e-4)
    assert _rel_err(bt.grad.cpu().numpy(), db) <= max(tol / 5, 1e-4)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_flat_buffer_step_on_two_half_batches_equals_full_batch(dtype):
    """The arithmetic of a 2-rank data-parallel step on one device: the engine's flat-buffer path
    (dp.FlatParams + qk_*_bwd_weight_acc + qk_adam_step_zero_grad) accumulating the gradients of two half
    batches must equal the same path run once on the concatenated batch -- and both must equal the oracle."""
    import qcnn_amd
    from oracle import oracle
    from qcnn_amd import dp
    F = qcnn_amd.functional
    dev = _dev()
    rng = np.random.RandomState(31)
    rnd = lambda a: torch.tensor(a).to(dtype).float().numpy()
    x = rnd(rng.randn(8, 40, 128).astype(np.float32))
    w0 = rnd((rng.randn(3, 32, 128) / 20).astype(np.float32))
    b0 = (0.1 * rng.randn(128)).astype(np.float32)
    dy = rnd(rng.randn(8, 40, 128).astype(np.float32))
    kw = dict(padding='same', activation='relu')

    def run(parts):
        kernel = torch.nn.Parameter(torch.tensor(w0, device=dev))
        bias = torch.nn.Parameter(torch.tensor(b0, device=dev))
        flat = dp.FlatParams([kernel, bias])
        m, v = torch.zeros_like(flat.param), torch.zeros_like(flat.param)
        dxs = []
        for lo, hi in parts:
            xt = torch.tensor(x[lo:hi], device=dev).to(dtype)
            dyt = torch.tensor(dy[lo:hi], device=dev).to(dtype)
            call = F.conv_call(tuple(xt.shape), tuple(kernel.shape), dtype, 1, 1, 'same', 'channels_last', 1, 'relu', True)
            y = call.fwd(xt, kernel.data, bias.data)
            call.bwd_weight(xt, dyt, y, True, out=(flat.grad_view(0), flat.grad_view(1)), accumulate=True)
            dxs.append(call.bwd_data(dyt, y, kernel.data))
        grad = flat.grad.clone()
        # "all-reduce" already happened (sum over the parts); 1/world folded into the optimiser like dp does
        F.adam_step(flat.param, flat.grad, m, v, 1, lr=1e-3, grad_scale=1.0 / len(parts), zero_grad=True)
        assert float(flat.grad.abs().max()) == 0.0
        return grad, flat.param.clone(), torch.cat(dxs).float(), flat

    g2, p2, dx2, flat = run([(0, 4), (4, 8)])
    g1, p1, dx1, _ = run([(0, 8)])
    tol = 1e-5 if dtype == torch.float32 else 2e-3
    assert _rel_err(g2.cpu().numpy(), g1.cpu().numpy()) <= tol
    assert _rel_err(dx2.cpu().numpy(), dx1.cpu().numpy()) <= tol
    y = oracle.forward(x, w0, b0, 1, **kw)
    dxo, dwo, dbo = oracle.backward(x, w0, b0, dy, 1, y=y, **kw)
    n_w = dwo.size
    otol = 1e-4 if dtype == torch.float32 else 2e-3
    assert _rel_err(g2[:n_w].cpu().numpy().reshape(dwo.shape), dwo) <= otol
    off_b = flat.offsets[1]
    assert _rel_err(g2[off_b:off_b + dbo.size].cpu().numpy(), dbo) <= otol
    # Adam with grad_scale = 1/2 on the summed gradient == Adam on the mean gradient: first step moves every weight
    # by lr * sign(g) (bias-corrected), so both runs must agree to rounding wherever |g| is not ~0
    big = g1.abs() > 1e-3 * g1.abs().max()
    assert float((p2 - p1)[big].abs().max()) <= 2e-4


CFG5_STACK = [('fp16', torch.float16), ('bf16', torch.bfloat16)]


@pytest.mark.parametrize('name,dtype', CFG5_STACK, ids=[c[0] for c in CFG5_STACK])
def test_cfg5_stack_small_matches_oracle(name, dtype):
    """BASELINE configs[4] per-GPU stack at a size the oracle finishes: QuaternionConv2D 1 -> 256 (tap-folded),
    2 x (256 -> 256) (3,5) 'same' relu as one chain, TimeDistributed(QuaternionDense(256)) head as an (F, 1) conj
    convolution; forward and all gradients against the oracle composition (16-bit storage emulated forward)."""
    import qcnn_amd
    from oracle import oracle
    F = qcnn_amd.functional
    dev = _dev()
    rng = np.random.RandomState(37)
    rnd = lambda a: torch.tensor(a).to(dtype).double().numpy()
    B, Fr, T = 1, 4, 8
    x = rnd(rng.randn(B, Fr, T, 4))
    shapes = [(3, 5, 1, 1024), (3, 5, 256, 1024), (3, 5, 256, 1024), (Fr, 1, 256, 256)]
    kws = [dict(padding='same', activation='relu')] * 3 + [dict(padding='valid', activation='relu', conj=True)]
    ws = [rnd(rng.randn(*s) / np.sqrt(np.prod(s[:-1]) * 4)) for s in shapes]
    bs = [0.1 * rng.randn(s[-1]).astype(np.float32).astype(np.float64) for s in shapes]
    acts = [x]
    for w, b, kw in zip(ws, bs, kws):
        acts.append(rnd(oracle.forward(acts[-1], w, b, 2, **kw)))
    dy = rnd(rng.randn(*acts[-1].shape))
    xt = torch.tensor(x, device=dev).to(dtype)
    wt = [torch.tensor(w, device=dev, dtype=torch.float32, requires_grad=True) for w in ws]
    bt = [torch.tensor(b, device=dev, dtype=torch.float32, requires_grad=True) for b in bs]
    h = F.quaternion_conv(xt, wt[0], bt[0], **kws[0])                     # first layer: no input gradient -> folded
    y = F.quaternion_conv_chain(h, [(wt[i], bt[i], kws[i]) for i in (1, 2, 3)])
    y.backward(torch.tensor(dy, device=dev).to(dtype))
    tol_y, tol_g = (4e-3, 1e-2) if dtype == torch.float16 else (2e-2, 5e-2)
    assert _rel_err(y.detach().float().cpu().numpy(), acts[-1]) <= tol_y
    # backward on the GPU's own activations (relu masks; with 8 - 32 rows per gradient element a single output that
    # rounds across zero moves a kernel-gradient element by tens of percent)
    acts = [x]
    with torch.no_grad():
        hh = xt
        for i in range(4):
            hh = F.quaternion_conv(hh, wt[i], bt[i], **kws[i])
            acts.append(hh.double().cpu().numpy())
    assert np.array_equal(acts[-1], y.detach().double().cpu().numpy())
    g = dy
    for i in reversed(range(4)):
        g, dw, db = oracle.backward(acts[i], ws[i], bs[i], g, 2, y=acts[i + 1], **kws[i])
        assert _rel_err(wt[i].grad.cpu().numpy(), dw) <= tol_g, 'dkernel %d' % i
        assert _rel_err(bt[i].grad.cpu().numpy(), db) <= tol_g, 'dbias %d' % i


def test_cfg5_stack_full_size_16bit_kernels_agree_with_exact_fp32_kernels():
    """BASELINE configs[4] at its per-GPU size (32 samples, 14 x 200, fp16): conv 1 -> 256 (folded), 2 x (256 -> 256)
    as a chain, head as an (F, 1) conj convolution -- the 16-bit MFMA kernels against the exact fp32-MFMA kernels
    (QK_DBG_NO_MFMA16) on the same 16-bit operands, end to end (output, every kernel gradient), plus checksums."""
    import qcnn_amd
    F = qcnn_amd.functional
    dev = _dev()
    dtype = torch.float16
    g = torch.Generator(device=dev).manual_seed(41)
    B, Fr, T = 32, 14, 200
    x = torch.randn(B, Fr, T, 4, device=dev, generator=g).to(dtype)
    shapes = [(3, 5, 1, 1024), (3, 5, 256, 1024), (3, 5, 256, 1024), (Fr, 1, 256, 256)]
    kws = [dict(padding='same', activation='relu')] * 3 + [dict(padding='valid', activation='relu', conj=True)]
    ws = [(torch.randn(s, device=dev, generator=g) / (2.0 * (s[0] * s[1] * s[2]) ** 0.5)).to(dtype).float() for s in shapes]
    bs = [(torch.randn(s[-1], device=dev, generator=g) / 10).to(dtype).float() for s in shapes]
    dy = torch.randn(B, 1, T, 256, device=dev, generator=g).to(dtype)

    def run():
        wt = [w.clone().requires_grad_(True) for w in ws]
        bt = [b.clone().requires_grad_(True) for b in bs]
        h = F.quaternion_conv(x, wt[0], bt[0], **kws[0])
        y = F.quaternion_conv_chain(h, [(wt[i], bt[i], kws[i]) for i in (1, 2, 3)])
        y.backward(dy)
        torch.cuda.synchronize()
        return [y.detach().float()] + [w.grad for w in wt] + [b.grad for b in bt]

    from qcnn_amd import _lib
    fast = run()
    with _lib.debug_flags(_lib.QK_DBG_NO_MFMA16):
        exact = run()
    assert not torch.equal(fast[2], exact[2]), 'QK_DBG_NO_MFMA16 did not switch kernels: the check is vacuous'
    for i, (a, e) in enumerate(zip(fast, exact)):
        err = float((a - e).abs().max()) / float(e.abs().max())
        # relu masks are decided by each path's own 16-bit y here and the gradient passes through three 16-bit
        # tensors before it reaches the first kernel: element-wise 3e-2, the checksums stay tight
        assert err <= (1e-2 if i == 0 else 3e-2), 'tensor %d: rel err %.3g' % (i, err)
        ssum = abs(float(a.double().sum()) - float(e.double().sum())) / float(e.double().abs().sum())
        # (bias gradients: 256 sums over 6400 rows each, gated by each path's own relu mask -- a handful of outputs
        # that round across zero move the checksum by ~1e-3)
        assert ssum <= (3e-3 if i >= 5 else 1e-3), 'tensor %d: checksum drift %.3g' % (i, ssum)


# ---- post-ops: PReLU + Dropout fused into the kernels (interspeech_model.py:99-101,117-121) ----------------------------
def _np_drop_factor(shape, seed, rate, idx=None):
    """The counter-based dropout mask of csrc/qk_postop.h restated in numpy: one 32-bit hash (+ one extra mixing round)
    per 16-byte unit of 8 elements of the flat channels_last tensor, 8 bits per element, keep iff bits >= round(rate * 256);
    kept elements are scaled by 256 / (256 - thr).  idx: the flat element indices to evaluate (an array of `shape`;
    default: all of a tensor of that shape) -- a window of a larger tensor keeps that tensor's indices."""
    if rate == 0:
        return np.ones(shape)
    n = int(np.prod(shape))
    idx = np.arange(n, dtype=np.uint64) if idx is None else np.asarray(idx, dtype=np.uint64).reshape(-1)
    M = np.uint64(0xffffffff)
    h = ((idx >> np.uint64(3)) ^ np.uint64(seed)) * np.uint64(0x9E3779B1) & M
    h ^= h >> np.uint64(15); h = h * np.uint64(0x85EBCA77) & M
    h ^= h >> np.uint64(13); h = h * np.uint64(0xC2B2AE3D) & M
    lo = h ^ (h >> np.uint64(16))
    hi = (lo ^ np.uint64(0x68E31DA4)) * np.uint64(0xB5297A4D) & M
    hi ^= hi >> np.uint64(15)
    e = idx & np.uint64(7)
    word = np.where(e < 4, lo, hi)
    v = (word >> (np.uint64(8) * (e & np.uint64(3)))) & np.uint64(0xff)
    thr = min(int(rate * 256 + 0.5), 255)
    return (np.where(v >= thr, 256.0 / (256.0 - thr), 0.0)).reshape(shape)


def _np_post(pre, alpha_b, keep):
    return (np.maximum(pre, 0) + alpha_b * np.minimum(pre, 0)) * keep


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16], ids=['fp32', 'bf16', 'fp16'])
@pytest.mark.parametrize('shape,axis', [((3, 5, 7, 16), 0), ((2, 6, 9, 32), 1), ((4, 11, 24), -1), ((50, 64), -1)],
                         ids=['axis0', 'axis1', 'scalar3d', 'scalar2d'])
def test_prelu_dropout_op_matches_numpy(shape, axis, dtype):
    """qk_postop_fwd / qk_postop_bwd on their own: values, d input, d alpha, with and without dropout."""
    import qcnn_amd
    F = qcnn_amd.functional
    dev = _dev()
    rng = np.random.RandomState(43)
    rnd = lambda a: torch.tensor(a).to(dtype).double().numpy()
    x = rnd(rng.randn(*shape))
    dy = rnd(rng.randn(*shape))
    alen = shape[1 + axis] if axis >= 0 else 1
    alpha = (0.05 + 0.3 * rng.rand(alen)).astype(np.float32)
    ab = alpha.astype(np.float64).reshape([alen if (axis >= 0 and i == 1 + axis) else 1 for i in range(len(shape))]) if axis >= 0 else alpha.astype(np.float64)[0]
    for rate, seed in ((0.0, 0), (0.3, 12345)):
        keep = _np_drop_factor(shape, seed, rate)
        want = _np_post(x, ab, keep)
        g = dy * keep
        want_dx = np.where(x > 0, g, np.where(x < 0, ab * g, 0.0))
        red = tuple(i for i in range(len(shape)) if not (axis >= 0 and i == 1 + axis))
        want_da = (g * np.minimum(x, 0)).sum(axis=red).reshape(-1)
        xt = torch.tensor(x, device=dev).to(dtype).requires_grad_(True)
        at = torch.tensor(alpha, device=dev, requires_grad=True)
        y = F.prelu_dropout(xt, at, axis, rate, seed)
        y.backward(torch.tensor(dy, device=dev).to(dtype))
        tol = 1e-6 if dtype == torch.float32 else (1e-2 if dtype == torch.bfloat16 else 2e-3)
        assert _rel_err(y.detach().float().cpu().numpy(), want) <= tol
        assert _rel_err(xt.grad.float().cpu().numpy(), want_dx) <= tol
        assert _rel_err(at.grad.cpu().numpy(), want_da) <= max(tol / 10, 1e-5)
        if rate:
            frac = float((keep == 0).mean())
            assert abs(frac - rate) < 0.05, frac               # the hash drops about `rate` of the elements


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('rate', [0.0, 0.25], ids=['nodrop', 'drop'])
def test_conv_chain_with_prelu_dropout_matches_oracle_composition(dtype, rate):
    """quaternion_conv_chain with post-ops (qk_conv_fwd_post / qk_conv_bwd_post: PReLU slopes per position of spatial
    axis 0, dropout masks regenerated from the seed) against the oracle's LINEAR layers + the numpy post-op:
    values, d input, every kernel / bias / slope gradient.  32 -> 32 -> 64 (band kernels), then a conj 'valid' head."""
    import qcnn_amd
    from oracle import oracle
    F = qcnn_amd.functional
    dev = _dev()
    rng = np.random.RandomState(47)
    rnd = (lambda a: a) if dtype == torch.float32 else (lambda a: torch.tensor(a).to(dtype).double().numpy())
    specs = [((3, 5, 32, 128), dict(padding='same', activation=None), 0),
             ((3, 5, 32, 256), dict(padding='same', activation=None), 0),
             ((6, 1, 64, 128), dict(padding='valid', activation=None, conj=True), -1)]
    x = rnd(rng.randn(2, 6, 40, 128).astype(np.float32).astype(np.float64))
    ws = [rnd((rng.randn(*s) / np.sqrt(np.prod(s[:-1]) * 4)).astype(np.float32).astype(np.float64)) for s, _, _ in specs]
    bs = [(0.1 * rng.randn(s[-1])).astype(np.float32).astype(np.float64) for s, _, _ in specs]
    alphas = [(0.05 + 0.3 * rng.rand(6 if ax == 0 else 1)).astype(np.float32) for _, _, ax in specs]
    seeds = [101, 202, 303]
    acts, pres, keeps = [x], [], []
    for w, b, (_, kw, ax), al, sd in zip(ws, bs, specs, alphas, seeds):
        pre = rnd(oracle.forward(acts[-1], w, b, 2, **kw))
        keep = _np_drop_factor(pre.shape, sd, rate)
        ab = al.astype(np.float64).reshape(1, -1, 1, 1) if ax == 0 else float(al[0])
        pres.append(pre); keeps.append(keep)
        acts.append(rnd(_np_post(pre, ab, keep)))
    dy = rnd(rng.randn(*acts[-1].shape).astype(np.float32).astype(np.float64))
    xt = torch.tensor(x, device=dev).to(dtype).requires_grad_(True)
    wt = [torch.tensor(w, device=dev, dtype=torch.float32, requires_grad=True) for w in ws]
    bt = [torch.tensor(b, device=dev, dtype=torch.float32, requires_grad=True) for b in bs]
    at = [torch.tensor(a, device=dev, requires_grad=True) for a in alphas]
    layers = [(wt[i], bt[i], dict(specs[i][1], post=dict(alpha=at[i], alpha_axis=specs[i][2], rate=rate, seed=seeds[i]))) for i in range(3)]
    y = F.quaternion_conv_chain(xt, layers)
    y.backward(torch.tensor(dy, device=dev).to(dtype))
    tol_y, tol_g = (1e-4, 2e-4) if dtype == torch.float32 else (1e-2, 3e-2)
    assert _rel_err(y.detach().float().cpu().numpy(), acts[-1]) <= tol_y
    g = dy
    for i in reversed(range(3)):
        ax = specs[i][2]
        ab = alphas[i].astype(np.float64).reshape(1, -1, 1, 1) if ax == 0 else float(alphas[i][0])
        gk = g * keeps[i]
        want_da = (gk * np.minimum(pres[i], 0)).sum(axis=(0, 2, 3)) if ax == 0 else np.array([(gk * np.minimum(pres[i], 0)).sum()])
        dpre = np.where(pres[i] > 0, gk, np.where(pres[i] < 0, ab * gk, 0.0))
        g, dw, db = oracle.backward(acts[i], ws[i], bs[i], dpre, 2, **specs[i][1])
        assert _rel_err(wt[i].grad.cpu().numpy(), dw) <= tol_g, 'dkernel %d' % i
        assert _rel_err(bt[i].grad.cpu().numpy(), db) <= tol_g, 'dbias %d' % i
        assert _rel_err(at[i].grad.cpu().numpy(), want_da) <= tol_g, 'dalpha %d' % i
    assert _rel_err(xt.grad.float().cpu().numpy(), g) <= tol_g


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16], ids=['fp32', 'bf16', 'fp16'])
def test_relu_dropout_op_matches_numpy(dtype):
    """The relu form of the post-op on its own (qk_postop_* with alpha == NULL): y = dropout(relu(x)); the backward is
    handed y only (d x = dy / (1 - rate) where y > 0)."""
    import qcnn_amd
    F = qcnn_amd.functional
    dev = _dev()
    rng = np.random.RandomState(44)
    rnd = lambda a: torch.tensor(a).to(dtype).double().numpy()
    for shape in ((3, 5, 7, 16), (50, 64)):
        x = rnd(rng.randn(*shape))
        dy = rnd(rng.randn(*shape))
        for rate, seed in ((0.0, 0), (0.3, 777)):
            keep = _np_drop_factor(shape, seed, rate)
            xt = torch.tensor(x, device=dev).to(dtype).requires_grad_(True)
            y = F.relu_dropout(xt, rate, seed)
            y.backward(torch.tensor(dy, device=dev).to(dtype))
            tol = 1e-6 if dtype == torch.float32 else (1e-2 if dtype == torch.bfloat16 else 2e-3)
            assert _rel_err(y.detach().float().cpu().numpy(), np.maximum(x, 0) * keep) <= tol
            assert _rel_err(xt.grad.float().cpu().numpy(), dy * keep * (x > 0)) <= tol


@pytest.mark.parametrize('flat', [False, True], ids=['autograd_grads', 'direct_flat_grads'])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('rate', [0.0, 0.25], ids=['nodrop', 'drop'])
def test_conv_chain_with_relu_dropout_matches_oracle_composition(dtype, rate, flat):
    """The aact='none' setting of the TIMIT model (relu + Dropout behind every body convolution,
    interspeech_model.py:117-121,131-137) as fused post-ops in their RELU form: each forward launch writes ONLY
    y = dropout(relu(W (x) x + b)); the next layer's backward-data epilogue multiplies by (y > 0) / (1 - rate).  Checked
    against the oracle's LINEAR layers + numpy relu / hash-mask: values, d input, every kernel / bias gradient.
    32 -> 32 -> 64 (band kernels), then a conj 'valid' head.  `flat`: the gradients are ADDED into dp.FlatParams views by
    the kernels (QK_BWD_ACCUMULATE through qk_conv_bwd_post) instead of returned to autograd."""
    import qcnn_amd
    from oracle import oracle
    F = qcnn_amd.functional
    dev = _dev()
    rng = np.random.RandomState(49)
    rnd = (lambda a: a) if dtype == torch.float32 else (lambda a: torch.tensor(a).to(dtype).double().numpy())
    specs = [((3, 5, 32, 128), dict(padding='same', activation=None)),
             ((3, 5, 32, 256), dict(padding='same', activation=None)),
             ((6, 1, 64, 128), dict(padding='valid', activation=None, conj=True))]
    x = rnd(rng.randn(2, 6, 40, 128).astype(np.float32).astype(np.float64))
    ws = [rnd((rng.randn(*s) / np.sqrt(np.prod(s[:-1]) * 4)).astype(np.float32).astype(np.float64)) for s, _ in specs]
    bs = [(0.1 * rng.randn(s[-1])).astype(np.float32).astype(np.float64) for s, _ in specs]
    seeds = [111, 222, 333]
    xt = torch.tensor(x, device=dev).to(dtype).requires_grad_(True)
    wt = [torch.nn.Parameter(torch.tensor(w, device=dev, dtype=torch.float32)) for w in ws]
    bt = [torch.nn.Parameter(torch.tensor(b, device=dev, dtype=torch.float32)) for b in bs]
    if flat:
        fp = qcnn_amd.dp.FlatParams([p for pair in zip(wt, bt) for p in pair], direct=True)
    layers = [(wt[i], bt[i], dict(specs[i][1], post=dict(alpha=None, rate=rate, seed=seeds[i]))) for i in range(3)]
    taps = []
    F.chain_tap = taps.append
    try:
        y = F.quaternion_conv_chain(xt, layers)
    finally:
        F.chain_tap = None
    # Forward, layer by layer ON THE GPU'S OWN INPUT of each layer: a 16-bit output that lands one ulp away from the
    # float64 value (y = relu(pre) * 4/3 is rounded once here, fp32-then-16-bit there) perturbs the next layer's
    # pre-activations by 1e-3 and flips relu decisions of elements near zero -- each flip is a full term of the
    # gradient.  Feeding every layer what the GPU fed it keeps the comparison element-wise.
    gpu = [t.detach().double().cpu().numpy() for t in taps[0]]
    assert len(gpu) == 4 and np.array_equal(gpu[0], x)
    tol_y, tol_g = (1e-4, 2e-4) if dtype == torch.float32 else (1e-2, 2e-2)
    keeps = []
    for i, (w, b, (_, kw), sd) in enumerate(zip(ws, bs, specs, seeds)):
        pre = oracle.forward(gpu[i], w, b, 2, **kw)
        keeps.append(_np_drop_factor(pre.shape, sd, rate))
        assert _rel_err(gpu[i + 1], rnd(np.maximum(pre, 0) * keeps[i])) <= tol_y, 'layer %d output' % i
    dy = rnd(rng.randn(*gpu[3].shape).astype(np.float32).astype(np.float64))
    y.backward(torch.tensor(dy, device=dev).to(dtype))
    if flat:
        assert all(p.grad.data_ptr() >= fp.grad.data_ptr() for p in wt + bt)
    g = dy
    for i in reversed(range(3)):
        dpre = g * keeps[i] * (gpu[i + 1] > 0)             # y > 0  <=>  pre > 0 and kept
        g, dw, db = oracle.backward(gpu[i], ws[i], bs[i], dpre, 2, **specs[i][1])
        assert _rel_err(wt[i].grad.cpu().numpy(), dw) <= tol_g, 'dkernel %d' % i
        assert _rel_err(bt[i].grad.cpu().numpy(), db) <= tol_g, 'dbias %d' % i
    assert _rel_err(xt.grad.float().cpu().numpy(), g) <= tol_g


def test_adam_step_folds_the_l2_term():
    """qk_adam_step_l2: g = grad * grad_scale + decay * param, then the Keras Adam update; zero_grad clears grad."""
    import qcnn_amd
    F = qcnn_amd.functional
    dev = _dev()
    rng = np.random.RandomState(5)
    n = 1000
    p0, g0 = rng.randn(n).astype(np.float32), rng.randn(n).astype(np.float32)
    dec = np.where(np.arange(n) < 600, 2 * 0.05, 0.0).astype(np.float32)
    p, g = torch.tensor(p0, device=dev), torch.tensor(g0, device=dev)
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    F.adam_step(p, g, m, v, 1, lr=1e-2, grad_scale=0.5, zero_grad=True, decay=torch.tensor(dec, device=dev))
    ge = g0.astype(np.float64) * 0.5 + dec.astype(np.float64) * p0
    me, ve = 0.1 * ge, 0.001 * ge * ge
    lr_t = 1e-2 * np.sqrt(1 - 0.999) / (1 - 0.9)
    want = p0 - lr_t * me / (np.sqrt(ve) + 1e-7)
    assert np.abs(p.cpu().numpy() - want).max() <= 1e-5 * np.abs(want).max()
    assert float(g.abs().max()) == 0.0 and _rel_err(m.cpu().numpy(), me) <= 1e-5


def test_fused_first_layer_declines_heights_whose_same_pooling_pads_low():
    """Round-2 advisor finding: TensorFlow's 'same' pooling with window = stride = 3 pads one row on the LOW side when
    H % 3 == 1 (e.g. 40 mel bins); the fused conv + pool kernels pool rows [3o, 3o + 2] and must decline those heights
    (C predicate and Python predicate agree), while the model's layer-by-layer path gives Keras' answer."""
    import qcnn_amd
    from qcnn_amd import _lib
    from qcnn_amd.models import TimitQCNN
    Fq = qcnn_amd.functional
    dev = _dev()
    for h, ok in ((41, True), (40, False), (39, True), (7, False), (8, True)):
        x = torch.randn(2, h, 30, 4, device=dev).to(torch.bfloat16)
        w = torch.randn(3, 5, 1, 128, device=dev)
        call = Fq.conv_call(tuple(x.shape), tuple(w.shape), x.dtype, 2, 1, 'same', 'channels_last', 1, 'relu', True, False)
        assert (int(_lib.lib().qk_conv_relu_pool_aux_bytes(ctypes.byref(call.desc), 3)) > 0) == ok, h
        assert Fq.conv_relu_pool_supported(x, w, 3) == ok, h
        if not ok:
            with pytest.raises(RuntimeError):
                Fq.conv_relu_pool(x, w, None, 3)
    np.random.seed(3); torch.manual_seed(3)
    m = TimitQCNN(num_layers=2, start_filter=32)
    x = torch.randn(2, 4, 40, 24, device=dev).to(torch.bfloat16)
    m.eval()
    with torch.no_grad():
        y = m(x)
        from qcnn_amd import _lib
        with _lib.debug_flags(_lib.QK_DBG_NO_FUSED_FIRST):            # the unfused composition (graph-level switch, include/qk.h)
            y2 = m(x)
        # Keras' first stage by hand: conv (relu) then max over TF 'same' windows of the 40 rows (lo pad 1)
        o = m.conv(x).float().cpu().numpy()                         # (B, C, 40, T)
        pooled, _ = _np_pool_h_same(np.moveaxis(o, 1, -1))          # (B, 14, T, C)
        got = m.pool(m.conv(x)).float().cpu().numpy()
    assert torch.equal(y, y2)
    assert pooled.shape[1] == 14 and np.array_equal(np.moveaxis(got, 1, -1), pooled)


# ---- the first TIMIT layer fused with its frequency pooling (qk_conv_relu_pool_*) ------------------------------------
def _np_pool_h_same(y, pool=3):
    """MaxPooling over axis 1, window = stride = pool, padding='same' with TensorFlow's rule (_shape.tf_pads: the low
    side gets total // 2 -- one row when H % 3 == 1)."""
    from qcnn_amd._shape import tf_pads
    n, h, w, c = y.shape
    lo, _ = tf_pads(h, pool, pool, 1, 'same')
    out = -(-h // pool)
    p = np.empty((n, out, w, c)); arg = np.empty((n, out, w, c), dtype=np.int64)
    for o in range(out):
        a, b = max(o * pool - lo, 0), min((o + 1) * pool - lo, h)
        seg = y[:, a:b]
        arg[:, o] = seg.argmax(1) + a
        p[:, o] = seg.max(1)
    return p, arg


@pytest.mark.parametrize('planes', [False, True], ids=['x_channels_last', 'x_component_planes'])
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'fp16'])
@pytest.mark.parametrize('shape,F', [((3, 41, 50, 4), 32), ((2, 9, 230, 4), 64), ((1, 8, 19, 4), 32),
                                     # round 6: filter counts that do not fill the kernel's 32-filter blocks (start_filter = 16 models)
                                     ((3, 41, 50, 4), 16), ((2, 9, 230, 4), 40), ((1, 8, 19, 4), 8)],
                         ids=['timit_small', 'two_chunks_two_column_tiles', 'partial_window_odd_width',
                              'sf16_half_block', 'f40_full_plus_quarter_block', 'f8_quarter_block'])
def test_fused_first_layer_conv_relu_pool_matches_oracle(shape, F, dtype, planes):
    """qk_conv_relu_pool_fwd / _bwd (conv (3,5) 'same' + relu + max-pool (3,1) 'same' over H, one kernel per direction,
    no pre-pool tensor) against oracle conv + numpy pooling: pooled values, d kernel, d bias.  Widths beyond one
    224-position chunk, two 32-filter column tiles and a partial last window are covered."""
    import qcnn_amd
    from oracle import oracle
    Fq = qcnn_amd.functional
    dev = _dev()
    rng = np.random.RandomState(53)
    rnd = lambda a: torch.tensor(a).to(dtype).double().numpy()
    x = rnd(rng.randn(*shape))
    w = rnd(rng.randn(3, 5, 1, 4 * F) / np.sqrt(60.0))
    b = (0.1 * rng.randn(4 * F)).astype(np.float32).astype(np.float64)
    kw = dict(padding='same', activation='relu')
    y = oracle.forward(x, w, b, 2, **kw)
    pooled, arg = _np_pool_h_same(y)
    dp = rnd(rng.randn(*pooled.shape))
    dy = np.zeros_like(y)
    n, ho, wd, c = pooled.shape
    ii = np.meshgrid(np.arange(n), np.arange(ho), np.arange(wd), np.arange(c), indexing='ij')
    np.add.at(dy, (ii[0], arg, ii[2], ii[3]), dp)
    _, dw, db = oracle.backward(x, w, b, dy, 2, y=y, **kw)
    xt = torch.tensor(x, device=dev).to(dtype)
    wt = torch.tensor(w, device=dev, dtype=torch.float32, requires_grad=True)
    bt = torch.tensor(b, device=dev, dtype=torch.float32, requires_grad=True)
    if planes:          # the reference's own input layout: (N, 4, H, W), the four component planes (interspeech_model.py:81)
        xt, lay = xt.permute(0, 3, 1, 2).contiguous(), 'channels_first'
    else:
        lay = 'channels_last'
    assert Fq.conv_relu_pool_supported(xt, wt, 3, lay)
    out = Fq.conv_relu_pool(xt, wt, bt, 3, lay)
    out.backward(torch.tensor(dp, device=dev).to(dtype))
    tol16, tol32 = (1e-2, 4e-3) if dtype == torch.bfloat16 else (2e-3, 2e-3)
    assert tuple(out.shape) == pooled.shape
    assert _rel_err(out.detach().float().cpu().numpy(), pooled) <= tol16
    assert _rel_err(wt.grad.cpu().numpy(), dw) <= tol32
    assert _rel_err(bt.grad.cpu().numpy(), db) <= tol32


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'fp16'])
@pytest.mark.parametrize('shape,F,per_row', [((3, 41, 50, 4), 32, True), ((2, 8, 230, 4), 64, True), ((2, 11, 33, 4), 32, False),
                                             ((3, 41, 50, 4), 16, True), ((2, 11, 33, 4), 40, False)],
                         ids=['41x50_f32', '8x230_f64', '11x33_scalar', '41x50_f16_half_block', '11x33_f40_scalar'])
@pytest.mark.parametrize('planes', [False, True], ids=['x_channels_last', 'x_component_planes'])
def test_fused_first_layer_conv_prelu_pool_matches_oracle(shape, F, per_row, dtype, planes):
    """qk_conv_prelu_pool_fwd / _bwd (linear conv (3,5) 'same' + PReLU with one slope per frequency row, or one slope +
    max-pool (3,1) 'same' over H, one kernel per direction) against oracle conv + numpy PReLU / pooling: pooled values,
    d kernel, d bias, d alpha.  Slopes of both signs (a negative slope makes PReLU non-monotonic: the maximum must be
    taken AFTER the activation)."""
    import qcnn_amd
    from oracle import oracle
    Fq = qcnn_amd.functional
    dev = _dev()
    rng = np.random.RandomState(61)
    rnd = lambda a: torch.tensor(a).to(dtype).double().numpy()
    x = rnd(rng.randn(*shape))
    w = rnd(rng.randn(3, 5, 1, 4 * F) / np.sqrt(60.0))
    b = (0.1 * rng.randn(4 * F)).astype(np.float32).astype(np.float64)
    H = shape[1]
    alpha = (0.5 * rng.randn(H if per_row else 1)).astype(np.float32).astype(np.float64)
    pre = oracle.forward(x, w, b, 2, padding='same', activation=None)
    a_b = alpha.reshape(1, -1, 1, 1) if per_row else alpha.reshape(1, 1, 1, 1)
    act = np.maximum(pre, 0) + a_b * np.minimum(pre, 0)
    pooled, arg = _np_pool_h_same(act)
    dp = rnd(rng.randn(*pooled.shape))
    dact = np.zeros_like(act)
    n, ho, wd, c = pooled.shape
    ii = np.meshgrid(np.arange(n), np.arange(ho), np.arange(wd), np.arange(c), indexing='ij')
    np.add.at(dact, (ii[0], arg, ii[2], ii[3]), dp)
    dpre = dact * np.where(pre > 0, 1.0, np.where(pre < 0, a_b, 0.0))
    dalpha = (dact * np.minimum(pre, 0)).sum(axis=(0, 2, 3)) if per_row else (dact * np.minimum(pre, 0)).sum().reshape(1)
    _, dw, db = oracle.backward(x, w, b, dpre, 2, padding='same', activation=None)
    xt = torch.tensor(x, device=dev).to(dtype)
    wt = torch.tensor(w, device=dev, dtype=torch.float32, requires_grad=True)
    bt = torch.tensor(b, device=dev, dtype=torch.float32, requires_grad=True)
    at = torch.tensor(alpha.reshape((1, H, 1) if per_row else (1, 1, 1)), device=dev, dtype=torch.float32, requires_grad=True)
    axis = 0 if per_row else -1
    lay = 'channels_last'
    if planes:
        xt, lay = xt.permute(0, 3, 1, 2).contiguous(), 'channels_first'
    assert Fq.conv_prelu_pool_supported(xt, wt, at, axis, 3, lay)
    out = Fq.conv_prelu_pool(xt, wt, bt, at, axis, 3, lay)
    out.backward(torch.tensor(dp, device=dev).to(dtype))
    tol16, tol32 = (1e-2, 5e-3) if dtype == torch.bfloat16 else (2e-3, 2e-3)
    assert tuple(out.shape) == pooled.shape
    assert _rel_err(out.detach().float().cpu().numpy(), pooled) <= tol16
    assert _rel_err(wt.grad.cpu().numpy(), dw) <= tol32
    assert _rel_err(bt.grad.cpu().numpy(), db) <= tol32
    # slope gradients are sums of terms of both signs: the error is measured against the sum of their magnitudes
    mag = np.abs(dact * np.minimum(pre, 0))
    scale = float(mag.sum(axis=(0, 2, 3)).max() if per_row else mag.sum())
    assert float(np.abs(at.grad.reshape(-1).cpu().numpy() - dalpha).max()) <= tol32 * scale


def test_cached_kernel_relayout_follows_every_kind_of_weight_update():
    """The 16-bit re-layout of a layer's kernel is kept on the parameter and reused (desc.ws_has_kernel = 1: no k_prep_w16
    launch) until the weights change.  Every way the weights can change must invalidate it: a torch in-place op on the
    parameter, the fused Adam kernel writing through a dp.FlatParams buffer, a torch op on that flat buffer, and re-homing the
    parameter's storage.  Reference: the same call with the cache switched off."""
    import qcnn_amd
    F = qcnn_amd.functional
    dev = _dev()
    dt = torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(5)
    x = torch.randn(2, 6, 40, 128, device=dev, generator=g).to(dt).requires_grad_(True)
    w = torch.nn.Parameter(torch.randn(3, 5, 32, 128, device=dev, generator=g) / 30)
    b = torch.nn.Parameter(torch.zeros(128, device=dev))
    dy = torch.randn(2, 6, 40, 128, device=dev, generator=g).to(dt)
    kw = dict(padding='same', activation=None)      # (a fused-relu layer's backward workspace also carries the masked dy: not cached)

    def run():
        x.grad = None
        y = F.quaternion_conv(x, w, b, **kw)
        y.backward(dy)
        return y.detach().clone(), x.grad.clone()

    def fresh():
        F._PREP_CACHE_ON = False
        try:
            return run()
        finally:
            F._PREP_CACHE_ON = True

    def check(what):
        got, want = run(), fresh()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), what
        return got
    y0 = check('first call')
    assert set(w._qk_prep) == {('f', 0, 1), ('t', 0, 1)}                       # forward and backward-data layouts are cached
    bufs = {k: v[2].data_ptr() for k, v in w._qk_prep.items()}
    y1 = check('second call: cache hit')
    assert {k: v[2].data_ptr() for k, v in w._qk_prep.items()} == bufs and torch.equal(y0[0], y1[0])
    with torch.no_grad():
        w.mul_(2.0)                                                          # torch in-place op on the parameter
    y2 = check('after w.mul_')
    assert not torch.equal(y2[0], y1[0])
    flat = qcnn_amd.dp.FlatParams([w, b], direct=True)                        # storage re-homed
    check('after re-homing into FlatParams')
    m, v = torch.zeros_like(flat.param), torch.zeros_like(flat.param)
    flat.grad.normal_(generator=g)
    F.adam_step(flat.param, flat.grad, m, v, 1, lr=1e-2, zero_grad=True)      # raw writes through the flat buffer
    y3 = check('after adam_step')
    with torch.no_grad():
        flat.param.mul_(0.5)                                                 # torch op on the flat buffer, not on the view
    y4 = check('after flat.param.mul_')
    assert not torch.equal(y4[0], y3[0])


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'fp16'])
def test_adam_step_with_16bit_layers_off_the_matrix_core_path(dtype):
    """Round-3 advisor (medium): the cached 16-bit kernel re-layouts were registered for EVERY trainable 16-bit layer, also
    those whose channel counts keep them off the matrix-core path (cq or fq not a multiple of 32); the batched refresh behind
    adam_step then failed with QK_ERR_UNSUPPORTED on the first optimiser step.  A model that mixes on-path and off-path
    layers must train: three steps, the loss goes down, the on-path layer's cache is refreshed, the off-path layers carry none."""
    import qcnn_amd
    from qcnn_amd import dp
    F = qcnn_amd.functional
    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(2)
    mk = lambda *s: torch.nn.Parameter(torch.randn(*s, device=dev, generator=g) / (4.0 * np.prod(s[:-1])) ** 0.5)
    w_small, w_path, w_dense = mk(3, 2, 4 * 16), mk(3, 16, 4 * 8), mk(8, 4 * 3)          # cq 2 -> fq 16, cq 16 -> fq 8, dense 8 -> 3
    w_on = mk(3, 32, 4 * 32)
    x = torch.randn(4, 30, 8, device=dev, generator=g).to(dtype)
    x_on = torch.randn(4, 30, 128, device=dev, generator=g).to(dtype)
    params = [w_small, w_path, w_dense, w_on]
    flat = dp.FlatParams(params, direct=True)
    m, v = torch.zeros_like(flat.param), torch.zeros_like(flat.param)
    losses = []
    for step in (1, 2, 3):
        h = F.quaternion_conv(x, w_small, None, padding='same', activation='relu', fold_small_cq=False)
        h = F.quaternion_conv(h, w_path, None, padding='same', activation='relu')
        y = F.quaternion_dense(h.reshape(-1, h.shape[-1]), w_dense, None)
        y_on = F.quaternion_conv(x_on, w_on, None, padding='same')
        loss = (y.float() ** 2).sum() + (y_on.float() ** 2).sum()
        loss.backward()
        losses.append(float(loss))
        F.adam_step(flat.param, flat.grad, m, v, step, lr=1e-2, zero_grad=True)          # raised here before the fix
    torch.cuda.synchronize()
    assert losses[2] < losses[0]
    assert not w_small.__dict__.get('_qk_prep') and not w_path.__dict__.get('_qk_prep') and not w_dense.__dict__.get('_qk_prep')
    cache = w_on.__dict__.get('_qk_prep')
    assert cache and all(ent[0] == (w_on._version, flat.param._version) for ent in cache.values())     # refreshed behind Adam
    # and the C entry point itself skips off-path jobs instead of refusing the whole batch
    call = F.conv_call((4, 30, 8), (3, 2, 64), dtype, 1, 1, 'same', 'channels_last', 1, None, False)
    job, op = call._prep_job(qcnn_amd._lib.QK_OP_FWD)
    ws = torch.empty(3 * 2 * 64 * 2 + 256, dtype=torch.uint8, device=dev)
    rc = qcnn_amd._lib.lib().qk_conv_prep_kernels(1, (ctypes.POINTER(qcnn_amd._lib.ConvDesc) * 1)(ctypes.pointer(job)), (ctypes.c_int32 * 1)(op),
                                                  (ctypes.c_void_p * 1)(w_small.data_ptr()), (ctypes.c_void_p * 1)(ws.data_ptr()),
                                                  torch.cuda.current_stream().cuda_stream)
    assert rc == 0


def _random_layer_configs(n, seed):
    """Seeded random layer configurations over everything the layer API accepts: rank 1-3 (+ dense), kernel extents 1-5,
    strides / dilations 1-2 (never both > 1, as in Keras), valid / same / causal, both data formats, with and without bias,
    relu / linear, channel counts on and off the 16-bit matrix-core path."""
    rng = np.random.RandomState(seed)
    out = []
    for i in range(n):
        rank = int(rng.choice([0, 1, 1, 2, 2, 3]))
        cq = int(rng.choice([1, 2, 3, 5, 8, 32]))
        fq = int(rng.choice([1, 2, 4, 32]))
        bias = bool(rng.rand() < 0.7)
        act = 'relu' if rng.rand() < 0.6 else None
        if rank == 0:
            out.append(('fuzz%02d_dense_%dx%d' % (i, cq, fq), 0, (int(rng.randint(1, 40)), 4 * cq), (cq, 4 * fq), dict(activation=act), bias))
            continue
        ks = tuple(int(rng.randint(1, 6 if rank < 3 else 4)) for _ in range(rank))
        if rng.rand() < 0.5:
            st, dl = tuple(int(rng.randint(1, 3)) for _ in range(rank)), (1,) * rank
        else:
            st, dl = (1,) * rank, tuple(int(rng.randint(1, 3)) for _ in range(rank))
        pad = str(rng.choice(['valid', 'same', 'causal'] if rank == 1 else ['valid', 'same']))
        sp = tuple(int(rng.randint((k - 1) * d + 1, (k - 1) * d + (14 if rank < 3 else 7))) for k, d in zip(ks, dl))
        fmt = str(rng.choice(['channels_last', 'channels_first']))
        bsz = int(rng.randint(1, 4))
        xs = (bsz, 4 * cq) + sp if fmt == 'channels_first' else (bsz,) + sp + (4 * cq,)
        kw = dict(strides=st, dilation_rate=dl, padding=pad, data_format=fmt, activation=act)
        out.append(('fuzz%02d_r%d_k%s_s%s_d%s_%s_%s_c%d_f%d' % (i, rank, 'x'.join(map(str, ks)), 'x'.join(map(str, st)), 'x'.join(map(str, dl)),
                                                               pad, 'cf' if fmt == 'channels_first' else 'cl', cq, fq), rank, xs, ks + (cq, 4 * fq), kw, bias))
    return out


FUZZ_CASES = _random_layer_configs(48, seed=2024)


@pytest.mark.parametrize('layout', ['channels_last', 'native'])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('case', FUZZ_CASES, ids=[c[0] for c in FUZZ_CASES])
def test_random_layer_configurations_match_oracle(case, dtype, layout):
    """48 seeded random layer configurations (see _random_layer_configs) x {fp32, bf16} x {internal channels-last, native
    layout}: output, d input, d kernel, d bias against the float64 oracle on the same operands -- the reference ships no
    tests, so breadth over its argument space is ours to supply."""
    import qcnn_amd
    _, rank, xs, ws, kw, bias = case
    x, w, b, dy, want = _oracle_case(rank, xs, ws, kw, seed=77, dtype=dtype, use_bias=bias)
    run = _run_native if layout == 'native' else _run_layer
    got = run(qcnn_amd.functional, x, w, b, dy, rank, dict(kw), dtype)
    tol16, tol32 = (1e-4, 1e-4) if dtype == torch.float32 else (1e-2, 3e-3)
    for k, v in got.items():
        err = _rel_err(v, want[k])
        if dtype == torch.float32 and kw.get('activation') == 'relu' and k != 'y' and err > 1e-4:
            # a pre-activation within float32 rounding of zero may flip its relu mask: compare on the GPU's own mask
            from oracle import oracle
            dxm, dwm, dbm = oracle.backward(x, w, b, dy * (got['y'] > 0), rank, **dict(kw, activation=None))
            err = _rel_err(v, dict(dx=dxm, dkernel=dwm, dbias=dbm)[k])
        assert err <= (tol16 if k in ('y', 'dx') else tol32), '%s: rel err %.3g (%s)' % (k, err, case[0])


def test_library_profiler_times_every_call_of_a_backward():
    """qk_prof_* (include/qk.h): with the recorder on, a layer's forward and its fused backward (backward-weight +
    backward-data inside ONE C call, on autograd's thread) leave three records carrying the layer's GEMM view, the
    kernel family that served them and a positive duration; off again, nothing is recorded."""
    import qcnn_amd
    from qcnn_amd import _lib
    F = qcnn_amd.functional
    dev = _dev()
    x = torch.randn(4, 14, 40, 128, device=dev).to(torch.bfloat16).requires_grad_(True)
    w = (torch.randn(3, 5, 32, 128, device=dev) / 20).requires_grad_(True)
    with _lib.profile() as p:
        y = F.quaternion_conv(x, w, None, padding='same', activation='relu')
        y.backward(torch.ones_like(y))
        torch.cuda.synchronize()
        recs = p.records()
    assert sorted(r['op'] for r in recs) == ['bwd_data', 'bwd_weight', 'fwd']
    for r in recs:
        assert (r['rows'], r['n'], r['k']) == (4 * 14 * 40, 128, 3 * 5 * 128) and r['ms'] > 0 and r['path'].startswith('mfma16')
    F.quaternion_conv(x, w, None, padding='same', activation='relu')
    assert _lib.lib().qk_prof_count() == 3


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [((6, 200, 160), (3, 40, 256)), ((2, 9, 31, 96), (3, 5, 24, 64))], ids=['conv1d_cfg2_small_batch', 'conv2d_24to16'])
def test_fp32_backward_weight_is_bit_repeatable_in_deterministic_mode(shape):
    """Round 6: k_wgrad<float> folds the 16 expanded blocks onto the 4 parts with a register reduce-scatter (DPP / ds_swizzle) and
    takes the bias sums from the staged registers -- both in a fixed order; with QK_DBG_DETERMINISTIC (one split of M, one owner per
    bias column) two runs must agree bit for bit, and the default (split, atomic) run with them to fp32 rounding."""
    import qcnn_amd
    from qcnn_amd import _lib
    F = qcnn_amd.functional
    dev = _dev()
    xs, ws = shape
    rank = len(xs) - 2
    g = torch.Generator(device=dev).manual_seed(5)
    x = torch.randn(xs, device=dev, generator=g)
    w = torch.randn(ws, device=dev, generator=g) / 20
    b = torch.randn(ws[-1], device=dev, generator=g) / 10
    call = F.conv_call(xs, ws, torch.float32, rank, 1, 'same', 'channels_last', 1, 'relu', True)
    y = call.fwd(x, w, b)
    dy = torch.randn(call.y_shape, device=dev, generator=g)

    def run(flags):
        with _lib.debug_flags(flags):
            dx, dw, db = call.bwd(x, dy, y, w, True)
            torch.cuda.synchronize()
        return dx, dw, db
    a = run(_lib.QK_DBG_DETERMINISTIC)
    c = run(_lib.QK_DBG_DETERMINISTIC)
    d = run(0)
    assert _lib.last_path() == 'fp32_mfma'
    for u, v in zip(a, c):
        assert torch.equal(u, v)
    for u, v in zip(a, d):
        assert float((u - v).abs().max()) <= 2e-5 * float(u.abs().max())
    assert float(a[1].abs().max()) > 0 and float(a[2].abs().max()) > 0
