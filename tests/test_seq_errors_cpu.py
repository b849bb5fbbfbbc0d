"""CPU: the argument checks of the sequence kernels' C entry points (include/qk_rnn.h, qk_norm.h, qk_attn.h, qk_dwconv.h,
qk_rnnt.h): return code and the full qk_last_error() text of every rejected call, and the path code of the smallest shapes that
select each kernel family.

tests/golden/g19_seq_errors.json holds {case id: [return value, message or null]}.  It was recorded once, with
{id: _run(fn) for id, fn in _cases()} over the same table, from a build of the commit BEFORE these five files got one shared
header for their vector I/O, launch check and host checks: the shared helpers must reproduce every code and every message.

No call here reaches a kernel launch.  The descriptor-level cases take no buffers.  The buffer-level cases pass made-up non-NULL
addresses to entry points whose check of exactly that argument precedes their first launch; they run only WITHOUT a GPU, where a
launch that slipped through a reordered check fails (and the test with it) instead of touching a made-up address."""
import ctypes
import json
import os

import pytest
import torch

from qcnn_amd import _lib as L
from conftest import GOLDEN

F32, BF16 = L.QK_F32, L.QK_BF16
P = 0x100000            # a made-up, 256-byte aligned, non-NULL address: never dereferenced


def _lstm(**kw):
    f = dict(dtype=BF16, batch=2, steps=3, q_units=16, directions=1, y_stride=64, flags=0)
    f.update(kw)
    return L.QLSTMDesc(**f)


def _lnorm(**kw):
    f = dict(dtype=BF16, rows=4, steps=0, q=8, x_stride=32, y_stride=32, flags=0)
    f.update(kw)
    return L.QLNormDesc(**f)


def _attn(**kw):
    f = dict(dtype=BF16, batch=2, steps=4, heads=2, dq=16, flags=0)
    f.update(kw)
    units = f['heads'] * f['dq']
    for n in 'qkvo':
        f.setdefault(n + '_row', 4 * units)
        f.setdefault(n + '_comp', units)
    return L.QAttnDesc(**f)


def _dwconv(**kw):
    f = dict(dtype=BF16, batch=2, steps=4, units=8, taps=3, pad_lo=1, flags=0)
    f.update(kw)
    for n in 'xy':
        f.setdefault(n + '_row', 4 * f['units'])
        f.setdefault(n + '_comp', f['units'])
    return L.QDWConvDesc(**f)


# family -> (descriptor builder, descriptor-only entry points, one out-of-range shape, an unknown flag, a row stride below its
# minimum, the shape of the vector / matrix path and its generic neighbour)
FAMILIES = {
    'qlstm': (_lstm, ('supported', 'workspace_bytes', 'reserve_bytes'), dict(batch=1, q_units=(1 << 16) + 1, y_stride=1 << 30),
              dict(flags=2), dict(y_stride=63), dict(q_units=16), dict(q_units=12, y_stride=48)),
    'qlnorm': (_lnorm, ('supported', 'slab_rows', 'workspace_bytes'), dict(q=(1 << 26) + 1), dict(flags=1), dict(x_stride=31),
               dict(q=8), dict(q=5, x_stride=20, y_stride=20)),
    'qattn': (_attn, ('supported', 'workspace_bytes'), dict(heads=65536, dq=1), dict(flags=1), dict(q_row=127), dict(dq=16),
              dict(dq=12)),
    'qdwconv': (_dwconv, ('supported', 'workspace_bytes'), dict(batch=65536), dict(flags=1), dict(x_row=31), dict(units=8),
                dict(units=5)),
}

# entry point -> (descriptor builder, argument names behind the descriptor, the buffers a valid call needs)
ENTRIES = {
    'qk_qlstm_fwd': (_lstm, 'zx R lengths h0 c0 y hT cT reserve workspace workspace_bytes stream', 'zx R y hT cT reserve workspace'),
    'qk_qlstm_bwd': (_lstm, 'dy dhT dcT R lengths h0 c0 y reserve dzx hprev dh0 dc0 workspace workspace_bytes stream',
                     'dy R y reserve dzx hprev dh0 dc0 workspace'),
    'qk_qlnorm_fwd': (_lnorm, 'x gamma beta lengths epsilon y stats stream', 'x y stats'),
    'qk_qlnorm_bwd': (_lnorm, 'dy x gamma lengths stats dx dgamma dbeta workspace workspace_bytes stream',
                      'dy x stats dx dgamma workspace'),
    'qk_qattn_fwd': (_attn, 'q k v lengths scale o lse stream', 'q k v o lse'),
    'qk_qattn_bwd': (_attn, 'd_o q k v o lse lengths scale d_q d_k d_v workspace workspace_bytes stream',
                     'd_o q k v o lse d_q d_k d_v workspace'),
    'qk_qdwconv_fwd': (_dwconv, 'a g w bias lengths y stream', 'a w y'),
    'qk_qdwconv_bwd': (_dwconv, 'dy a g w lengths da dg dw dbias workspace workspace_bytes stream', 'dy a w da dw workspace'),
}
RNNT = dict(B=2, T=3, U1=4, V=5)


def _ws_fn(entry):
    return getattr(L.lib(), entry[:entry.rindex('_')] + '_workspace_bytes')


def _entry_call(entry, dtype=BF16, **over):
    """entry(descriptor, made-up buffers ...) with the arguments in `over` replaced; workspace_bytes defaults to what the call needs.
    A call with nothing replaced would launch: every case replaces the one argument whose check it pins."""
    make, names, needed = ENTRIES[entry]
    desc = make(dtype=dtype)
    op = L.QK_OP_FWD if entry.endswith('_fwd') else L.QK_OP_BWD
    args = {n: None for n in names.split()}
    args.update({n: P + 0x1000 * i for i, n in enumerate(needed.split())})
    args.update(epsilon=1e-3, scale=0.0, workspace_bytes=int(_ws_fn(entry)(ctypes.byref(desc), op)))
    short, null_desc = over.pop('short', 0), over.pop('null_desc', False)
    args.update(over)
    args['workspace_bytes'] -= short
    return getattr(L.lib(), entry)(None if null_desc else ctypes.byref(desc), *[args[n] for n in names.split()])


def _rnnt_call(dtype=BF16, short=0, shape=None, **over):
    lib = L.lib()
    s = dict(RNNT, **(shape or {}))
    args = dict(logits=P, labels=P + 0x1000, input_length=P + 0x2000, label_length=P + 0x3000, cost=P + 0x4000, grad=P + 0x5000,
                workspace=P + 0x6000)
    args.update(over)
    need = int(lib.qk_rnnt_workspace_bytes(s['B'], s['T'], s['U1'], s['V']))
    return lib.qk_rnnt_loss(dtype, s['B'], s['T'], s['U1'], s['V'], args['logits'], args['labels'], args['input_length'],
                            args['label_length'], args['cost'], args['grad'], args['workspace'], need - short, None)


def _cases():
    """[(id, needs made-up buffers, callable -> return value)]"""
    cases = []

    def add(name, fn, buffers=False):
        cases.append((name, buffers, fn))

    def desc_fn(fam, ep, desc):
        fn = getattr(L.lib(), 'qk_%s_%s' % (fam, ep))
        ref = ctypes.byref(desc) if desc is not None else None
        return (lambda: fn(ref, L.QK_OP_BWD)) if ep == 'workspace_bytes' else (lambda: fn(ref))

    for fam, (make, eps, big, flag, stride, fast, generic) in FAMILIES.items():
        for ep in eps:
            for what, desc in (('null_desc', None), ('dtype3', make(dtype=3)), ('range', make(**big)), ('flags', make(**flag)),
                               ('stride', make(**stride))):
                add('%s_%s_%s' % (fam, ep, what), desc_fn(fam, ep, desc))
        ws = getattr(L.lib(), 'qk_%s_workspace_bytes' % fam)
        add(fam + '_workspace_bytes_op7', lambda ws=ws, d=make(): ws(ctypes.byref(d), 7))
        for dt, dn in ((BF16, 'bf16'), (F32, 'f32')):
            add('%s_path_fast_%s' % (fam, dn), desc_fn(fam, 'supported', make(dtype=dt, **fast)))
            add('%s_path_generic_%s' % (fam, dn), desc_fn(fam, 'supported', make(dtype=dt, **generic)))

    lib = L.lib()
    limits = dict(ok=(2, 3, 4, 5), v_max=(2, 3, 4, L.QK_RNNT_MAX_CLASSES), v_over=(2, 3, 4, L.QK_RNNT_MAX_CLASSES + 1),
                  u1_max=(2, 3, L.QK_RNNT_MAX_U1, 5), u1_over=(2, 3, L.QK_RNNT_MAX_U1 + 1, 5), v_1=(2, 3, 4, 1), b_0=(0, 3, 4, 5),
                  rows_2p31=(1 << 15, 1 << 15, 2, 5))
    for name, shape in limits.items():
        add('rnnt_supported_' + name, lambda s=shape: lib.qk_rnnt_supported(BF16, *s))
        add('rnnt_workspace_bytes_' + name, lambda s=shape: lib.qk_rnnt_workspace_bytes(*s))
    add('rnnt_supported_dtype3', lambda: lib.qk_rnnt_supported(3, 2, 3, 4, 5))

    for entry, (_, names, needed) in ENTRIES.items():
        first = needed.split()[0]
        lstm = 'qlstm' in entry
        add(entry + '_null_desc', lambda e=entry: _entry_call(e, null_desc=True))
        add(entry + '_null_buffer', lambda e=entry, n=first: _entry_call(e, **{n: None}), True)
        if lstm:        # 16 bytes for the activations, whatever the dtype
            add(entry + '_misaligned_8', lambda e=entry, n=first: _entry_call(e, **{n: P + 8}), True)
            add(entry + '_misaligned_R', lambda e=entry: _entry_call(e, R=P + 0x1000 + 2), True)
        else:
            add(entry + '_misaligned_bf16', lambda e=entry, n=first: _entry_call(e, **{n: P + 1}), True)
            add(entry + '_misaligned_f32', lambda e=entry, n=first: _entry_call(e, F32, **{n: P + 2}), True)
        if 'workspace' in names:
            add(entry + '_workspace_misaligned', lambda e=entry: _entry_call(e, workspace=P + 8), True)
            add(entry + '_workspace_null', lambda e=entry: _entry_call(e, workspace=None), True)
            add(entry + '_workspace_short', lambda e=entry: _entry_call(e, short=1), True)
            add(entry + '_workspace_short_f32', lambda e=entry: _entry_call(e, F32, short=1), True)
    add('qk_rnnt_loss_dtype3', lambda: _rnnt_call(3))
    add('qk_rnnt_loss_v_over', lambda: _rnnt_call(shape=dict(V=L.QK_RNNT_MAX_CLASSES + 1)))
    add('qk_rnnt_loss_null_buffer', lambda: _rnnt_call(logits=None), True)
    add('qk_rnnt_loss_misaligned_bf16', lambda: _rnnt_call(logits=P + 1), True)
    add('qk_rnnt_loss_misaligned_f32', lambda: _rnnt_call(F32, logits=P + 2), True)
    add('qk_rnnt_loss_workspace_misaligned', lambda: _rnnt_call(workspace=P + 0x6000 + 8), True)
    add('qk_rnnt_loss_workspace_null', lambda: _rnnt_call(workspace=None), True)
    add('qk_rnnt_loss_workspace_short', lambda: _rnnt_call(short=1), True)
    assert len({c[0] for c in cases}) == len(cases)
    return cases


def _run(fn):
    """[return value, message]: the message only where the call reports failure (0 from a size or path query, a negative status)."""
    rc = int(fn())
    return [rc, L.lib().qk_last_error().decode() if rc <= 0 else None]


@pytest.fixture(scope='module')
def recorded():
    with open(os.path.join(GOLDEN, 'g19_seq_errors.json')) as f:
        return json.load(f)


def test_the_table_is_the_recorded_one(recorded):
    assert sorted(recorded) == sorted(c[0] for c in _cases())
    assert all(msg for rc, msg in recorded.values() if rc <= 0), 'every failure was recorded with its message'


@pytest.mark.parametrize('buffers', [False, True], ids=['descriptor_level', 'buffer_level'])
def test_codes_and_messages_are_the_recorded_ones(recorded, buffers):
    if buffers and torch.cuda.is_available():
        pytest.skip('made-up addresses are only passed where no kernel can run')
    got = {name: _run(fn) for name, with_buffers, fn in _cases() if with_buffers == buffers}
    assert got
    wrong = {name: (got[name], recorded[name]) for name in got if got[name] != recorded[name]}
    assert not wrong, wrong


def test_every_kind_of_rejection_is_in_the_table(recorded):
    """The recorded table covers what it claims to: each status code, each family's both paths, the workspace figures."""
    codes = {rc for rc, _ in recorded.values()}
    assert {L.QK_ERR_INVALID_ARG, L.QK_ERR_UNSUPPORTED, L.QK_ERR_WORKSPACE, 0, 1, 2} <= codes
    for fam in FAMILIES:
        assert recorded['%s_path_fast_bf16' % fam][0] == 2 and recorded['%s_path_generic_bf16' % fam][0] == 1
    short = [msg for name, (rc, msg) in recorded.items() if name.endswith('_workspace_short')]
    assert len(short) == 6 and all(' bytes needed, ' in m for m in short)
