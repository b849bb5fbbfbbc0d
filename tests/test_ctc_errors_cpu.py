"""CPU: the argument checks of the CTC family's C entry points (include/qk.h: the CTC cost, CTC decoding, CTC forced alignment,
scoring alignment) and of their Python wrappers: return code and the full qk_last_error() text of every rejected call, exception
type and text of every refusal the wrappers make on CPU tensors, and ctc_shape_supported / ctc_supported around their limits.

tests/golden/g20_ctc_errors.json holds {case id: [return value, message]} for the C cases and {case id: [exception type, text]} or
{case id: value} for the Python ones.  It was recorded once, with {id: _run(fn)} over the same tables, from a build of the commit
BEFORE the CTC files got their shared lattice header, one LDS opt-in and by_dtype: the shared helpers must reproduce every code,
every message and the order in which the checks fire (the cases named *_then_* break two checks at once).

Some rejections set no message (a size query that returns 0, a launcher that refuses a dtype): _run() first makes a call with a
known message, so such a case records that the text was left alone.

No call here reaches a kernel launch.  The cases marked `buffers` pass made-up non-NULL addresses that no check dereferences;
they run only WITHOUT a GPU, where a launch that slipped through a reordered check fails (and the test with it) instead of
touching a made-up address.  One branch cannot be reached from outside and has no case: qk_ctc_beam_search_decode_lm's "LM rows
exceed the LDS budget" (every shape that passes the checks in front of it fits)."""
import json
import os
import types

import pytest
import torch

from qcnn_amd import _lib as L
from qcnn_amd import functional as F
from conftest import GOLDEN

F32, BF16 = L.QK_F32, L.QK_BF16
P = 0x100000            # a made-up, 256-byte aligned, non-NULL address: never dereferenced
NAN, INF = float('nan'), float('inf')

# entry point -> (argument names in order, the pointer arguments a valid call passes, the other arguments of a valid call)
ENTRIES = {
    'qk_ctc_batch_cost': ('dtype batch frames classes y_pred labels max_label_len input_length label_length cost dy_pred workspace '
                          'workspace_bytes stream', 'y_pred labels input_length label_length cost dy_pred workspace',
                          dict(dtype=BF16, batch=2, frames=8, classes=5, max_label_len=3)),
    'qk_ctc_greedy_decode': ('dtype batch frames classes y_pred input_length decoded decoded_len log_prob stream',
                             'y_pred input_length decoded decoded_len log_prob', dict(dtype=BF16, batch=2, frames=8, classes=5)),
    'qk_ctc_beam_search_decode': ('dtype batch frames classes y_pred input_length beam_width top_paths merge_repeated decoded '
                                  'decoded_len log_prob workspace workspace_bytes stream',
                                  'y_pred input_length decoded decoded_len log_prob workspace',
                                  dict(dtype=BF16, batch=2, frames=8, classes=5, beam_width=4, top_paths=2, merge_repeated=1)),
    'qk_ctc_beam_search_decode_lm': ('dtype batch frames classes y_pred input_length beam_width top_paths merge_repeated lm_order '
                                     'lm_table lm_weight insertion_bonus lm_eos decoded decoded_len log_prob score workspace '
                                     'workspace_bytes stream', 'y_pred input_length lm_table decoded decoded_len log_prob score workspace',
                                     dict(dtype=BF16, batch=2, frames=8, classes=5, beam_width=4, top_paths=2, merge_repeated=1,
                                          lm_order=2, lm_weight=0.5, insertion_bonus=0.25, lm_eos=1)),
    'qk_edit_distance': ('batch hyp hyp_stride hyp_len ref ref_stride ref_len class_map classes distance ref_len_out stream',
                         'hyp hyp_len ref ref_len distance ref_len_out', dict(batch=2, hyp_stride=6, ref_stride=5, classes=0)),
    'qk_edit_align': ('batch hyp hyp_stride hyp_len ref ref_stride ref_len class_map classes counts ali_ref ali_hyp ali_len confusion '
                      'out_classes workspace workspace_bytes stream',
                      'hyp hyp_len ref ref_len counts ali_ref ali_hyp ali_len workspace',
                      dict(batch=2, hyp_stride=6, ref_stride=5, classes=0, out_classes=0)),
    'qk_ctc_forced_align': ('dtype batch frames classes y_pred labels max_label_len input_length label_length path starts ends score '
                            'workspace workspace_bytes stream',
                            'y_pred labels input_length label_length path starts ends score workspace',
                            dict(dtype=BF16, batch=2, frames=8, classes=5, max_label_len=3)),
}


def _need(entry, a):
    lib = L.lib()
    if entry == 'qk_ctc_batch_cost':
        return lib.qk_ctc_workspace_bytes(a['batch'], a['frames'], a['max_label_len'])
    if entry.startswith('qk_ctc_beam'):
        return lib.qk_ctc_beam_workspace_bytes(a['batch'], a['frames'], a['beam_width'])
    if entry == 'qk_edit_align':
        return lib.qk_edit_align_workspace_bytes(a['batch'], a['hyp_stride'], a['ref_stride'])
    if entry == 'qk_ctc_forced_align':
        return lib.qk_ctc_align_workspace_bytes(a['batch'], a['frames'], a['max_label_len'])
    return 0


def _call(entry, nulls=False, short=0, **over):
    """entry(...) of a valid call with the arguments in `over` replaced: made-up addresses for the pointers (nulls: NULL for all of
    them), workspace_bytes what the replaced shape needs, less `short`.  A call with nothing replaced would launch: every case
    replaces the arguments whose checks it pins."""
    names, pointers, scalars = ENTRIES[entry]
    args = {n: None for n in names.split()}
    if not nulls:
        args.update({n: P + 0x1000 * i for i, n in enumerate(pointers.split())})
    args.update(scalars)
    args.update(over)
    if 'workspace_bytes' in args:
        args['workspace_bytes'] = max(int(_need(entry, args)) - short, 0)
    return getattr(L.lib(), entry)(*[args[n] for n in names.split()])


HUGE = dict(batch=1 << 15, frames=1 << 15, classes=2)          # batch x frames x classes = 2^31


def _c_cases():
    """[(id, passes made-up buffers, callable -> return value)]"""
    cases = []

    def add(name, fn, buffers=False):
        cases.append((name, buffers, fn))

    def entry(e, name, buffers=True, **over):
        add('%s_%s' % (e, name), lambda: _call(e, nulls=not buffers, **over), buffers)

    def null_each(e, names, **over):
        for n in names.split():
            entry(e, 'null_' + n, **dict(over, **{n: None}))

    def workspace(e, misaligned, **shape):
        entry(e, 'workspace_null', workspace=None, **shape)
        entry(e, 'workspace_short', short=1, **shape)
        entry(e, 'workspace_misaligned', workspace=P + 0x8000 + misaligned, **shape)

    lib = L.lib()
    for fn in ('qk_ctc_workspace_bytes', 'qk_ctc_beam_workspace_bytes', 'qk_ctc_align_workspace_bytes'):
        for name, shape in dict(ok=(2, 8, 3), batch_0=(0, 8, 3), frames_0=(2, 0, 3), third_0=(2, 8, 0), third_neg=(2, 8, -1),
                                all_bad=(-1, -1, -1)).items():
            add('%s_%s' % (fn, name), lambda fn=fn, s=shape: getattr(lib, fn)(*s))
    for name, shape in dict(ok=(2, 6, 5), batch_0=(0, 6, 5), hyp_neg=(2, -1, 5), ref_neg=(2, 6, -1), hyp_1025=(2, 1025, 5),
                            ref_1025=(2, 6, 1025), strides_0=(2, 0, 0), max=(1, 1024, 1024)).items():
        add('qk_edit_align_workspace_bytes_' + name, lambda s=shape: lib.qk_edit_align_workspace_bytes(*s))

    e = 'qk_ctc_batch_cost'
    for name, over in dict(batch_0=dict(batch=0), frames_0=dict(frames=0), classes_1=dict(classes=1),
                           labels_neg=dict(max_label_len=-1)).items():
        entry(e, 'extents_' + name, buffers=False, **over)
    entry(e, 'extents_then_null', batch=0, y_pred=None)
    null_each(e, 'y_pred labels input_length label_length cost')
    entry(e, 'null_then_workspace', cost=None, short=1)
    entry(e, 'no_labels_no_gradient_then_workspace', max_label_len=0, labels=None, dy_pred=None, short=1)
    workspace(e, 2)
    entry(e, 'workspace_then_2p31', short=1, **HUGE)
    entry(e, '2p31', **HUGE)
    entry(e, '2p31_then_limits', max_label_len=128, **HUGE)
    entry(e, 'labels_128', max_label_len=128)
    entry(e, 'classes_257', classes=257)
    entry(e, 'frames_for_lds', frames=17000)
    entry(e, 'dtype_3', dtype=3)
    entry(e, 'dtype_neg', dtype=-1)
    entry(e, 'limits_then_dtype', dtype=3, max_label_len=128)
    entry(e, 'workspace_then_dtype', dtype=3, short=1)

    e = 'qk_ctc_greedy_decode'
    for name, over in dict(batch_0=dict(batch=0), frames_0=dict(frames=0), classes_1=dict(classes=1), dtype_3=dict(dtype=3),
                           dtype_neg=dict(dtype=-1)).items():
        entry(e, 'bad_' + name, buffers=False, **over)
    entry(e, 'bad_then_classes', dtype=3, classes=257)
    null_each(e, 'y_pred input_length decoded decoded_len log_prob')
    entry(e, 'null_then_classes', classes=257, log_prob=None)
    entry(e, 'classes_257', classes=257)
    entry(e, 'classes_then_2p31', batch=1 << 15, frames=1 << 15, classes=257)
    entry(e, '2p31', **HUGE)

    for e in ('qk_ctc_beam_search_decode', 'qk_ctc_beam_search_decode_lm'):
        for name, over in dict(batch_0=dict(batch=0), frames_0=dict(frames=0), classes_1=dict(classes=1), beam_0=dict(beam_width=0),
                               paths_0=dict(top_paths=0), dtype_3=dict(dtype=3), dtype_neg=dict(dtype=-1)).items():
            entry(e, 'bad_' + name, buffers=False, **over)
        entry(e, 'bad_then_null', batch=0, y_pred=None)
        null_each(e, 'y_pred input_length decoded decoded_len log_prob')
        entry(e, 'null_then_unsupported', decoded=None, beam_width=129)
        entry(e, 'classes_257', classes=257)
        entry(e, 'beam_129', beam_width=129)
        entry(e, 'paths_over_beam', top_paths=5)
        entry(e, 'unsupported_then_2p31', beam_width=129, **HUGE)
        entry(e, '2p31_classes', **HUGE)
        entry(e, '2p31_paths', batch=1 << 14, frames=1 << 15, classes=2, beam_width=8, top_paths=8)
        entry(e, '2p31_then_workspace', short=1, **HUGE)
        workspace(e, 2)
    e = 'qk_ctc_beam_search_decode_lm'
    entry(e, 'bad_then_weight', buffers=False, batch=0, lm_weight=-1.0)
    for name, over in dict(weight_neg=dict(lm_weight=-0.5), weight_nan=dict(lm_weight=NAN), weight_inf=dict(lm_weight=INF),
                           bonus_inf=dict(insertion_bonus=-INF), bonus_nan=dict(insertion_bonus=NAN)).items():
        entry(e, name, buffers=False, **over)
    entry(e, 'weight_then_order', buffers=False, lm_weight=-1.0, lm_order=4)
    entry(e, 'order_0', buffers=False, lm_order=0)
    entry(e, 'order_4', buffers=False, lm_order=4)
    entry(e, 'order_then_null', lm_order=4, y_pred=None)
    null_each(e, 'score lm_table')
    entry(e, 'trigram_classes_65', lm_order=3, classes=65)
    entry(e, 'unsupported_then_trigram', lm_order=3, classes=65, beam_width=129)
    entry(e, 'trigram_then_2p31', lm_order=3, batch=1 << 15, frames=1 << 15, classes=65)
    entry(e, 'largest_lm_rows_then_workspace', classes=256, beam_width=128, short=1)

    e = 'qk_edit_distance'
    for name, over in dict(batch_0=dict(batch=0), hyp_neg=dict(hyp_stride=-1), ref_neg=dict(ref_stride=-1)).items():
        entry(e, 'bad_' + name, buffers=False, **over)
    entry(e, 'bad_class_map_without_classes', class_map=P + 0x9000, classes=0)
    entry(e, 'bad_then_null', batch=0, distance=None)
    null_each(e, 'hyp hyp_len ref ref_len distance')
    entry(e, 'null_then_ref_1025', ref_stride=1025, hyp_len=None)
    entry(e, 'ref_1025', ref_stride=1025)
    entry(e, 'no_tokens_no_ref_len_out_then_ref_1025', hyp_stride=0, hyp=None, ref_len_out=None, ref_stride=1025)

    e = 'qk_edit_align'
    for name, over in dict(batch_neg=dict(batch=-1), hyp_neg=dict(hyp_stride=-1), ref_neg=dict(ref_stride=-1)).items():
        entry(e, 'bad_' + name, buffers=False, **over)
    entry(e, 'bad_class_map_without_classes', class_map=P + 0x9000, classes=0)
    entry(e, 'bad_confusion_classes_neg', confusion=P + 0xa000, out_classes=-1)
    entry(e, 'bad_then_unsupported', buffers=False, batch=-1, hyp_stride=1025)
    entry(e, 'hyp_1025', buffers=False, hyp_stride=1025)
    entry(e, 'ref_1025', buffers=False, ref_stride=1025)
    entry(e, 'confusion_classes_257', confusion=P + 0xa000, out_classes=257)
    entry(e, 'unsupported_then_batch_0', buffers=False, batch=0, ref_stride=1025)
    entry(e, 'batch_0', buffers=False, batch=0)
    entry(e, 'batch_0_out_classes_without_confusion', buffers=False, batch=0, out_classes=257)
    entry(e, 'unsupported_then_null', ref_stride=1025, counts=None)
    null_each(e, 'hyp hyp_len ref ref_len counts')
    entry(e, 'null_then_trio', counts=None, ali_len=None)
    entry(e, 'trio_ref_only', ali_hyp=None, ali_len=None)
    entry(e, 'trio_no_len', ali_len=None)
    entry(e, 'trio_no_ref', ali_ref=None)
    long_pair = dict(hyp_stride=1024, ref_stride=1024)      # short pairs keep their table in LDS and need no workspace
    entry(e, 'trio_then_workspace', ali_hyp=None, short=1, **long_pair)
    entry(e, 'counts_only_then_workspace', ali_ref=None, ali_hyp=None, ali_len=None, short=1, **long_pair)
    workspace(e, 4, **long_pair)

    e = 'qk_ctc_forced_align'
    for name, over in dict(batch_0=dict(batch=0), frames_0=dict(frames=0), classes_1=dict(classes=1),
                           labels_neg=dict(max_label_len=-1)).items():
        entry(e, 'extents_' + name, buffers=False, **over)
    entry(e, 'extents_then_unsupported', buffers=False, batch=0, dtype=3)
    for name, over in dict(classes_257=dict(classes=257), labels_128=dict(max_label_len=128), dtype_3=dict(dtype=3),
                           dtype_neg=dict(dtype=-1)).items():
        entry(e, 'unsupported_' + name, buffers=False, **over)
    entry(e, 'unsupported_then_null', classes=257, y_pred=None)
    null_each(e, 'y_pred labels input_length label_length path starts ends score')
    entry(e, 'null_then_2p31', score=None, **HUGE)
    entry(e, 'no_labels_then_workspace', max_label_len=0, labels=None, starts=None, ends=None, short=1)
    entry(e, '2p31', **HUGE)
    entry(e, '2p31_then_frames', batch=1 << 14, frames=1 << 17, classes=2)
    entry(e, 'frames_for_lds', frames=40000)
    entry(e, 'frames_then_workspace', frames=40000, short=1)
    workspace(e, 4)
    assert len({c[0] for c in cases}) == len(cases)
    return cases


def _run(fn):
    """[return value, message]; the message is the marker's where the call set none."""
    lib = L.lib()
    assert lib.qk_ctc_greedy_decode(F32, 0, 0, 0, None, None, None, None, None, None) == L.QK_ERR_INVALID_ARG      # the marker
    return [int(fn()), lib.qk_last_error().decode()]


# ---- the Python wrappers on CPU tensors ---------------------------------------------------------------------------------------------
def _py_cases():
    """[(id, callable)]: a refusal is recorded as [exception type, text], a value as it is."""
    y = torch.full((2, 8, 5), 0.2)
    lab = torch.zeros((2, 3), dtype=torch.int64)
    il, ll = torch.tensor([8, 6]), torch.tensor([3, 2])
    lm = types.SimpleNamespace(order=2, num_labels=4)
    hyp, ref = torch.zeros((2, 6), dtype=torch.int64), torch.zeros((2, 5), dtype=torch.int64)
    hl, rl = torch.tensor([6, 2]), torch.tensor([5, 1])
    conf = torch.zeros((5, 5), dtype=torch.int32)
    cases = []

    def add(name, fn):
        cases.append((name, fn))

    add('ctc_batch_cost_cpu', lambda: F.ctc_batch_cost(y, lab, il, ll))
    add('ctc_batch_cost_cpu_then_loss_scale', lambda: F.ctc_batch_cost(y, lab, il, ll, loss_scale=-1.0))
    add('ctc_cost_and_grad_cpu', lambda: F.ctc_cost_and_grad(y, lab, il, ll))
    add('ctc_greedy_decode_cpu', lambda: F.ctc_greedy_decode(y, il))
    add('ctc_greedy_decode_cpu_then_shape', lambda: F.ctc_greedy_decode(y[0], il))
    add('ctc_greedy_decode_cpu_then_input_length', lambda: F.ctc_greedy_decode(y, torch.tensor([8, 6, 4])))

    def lm_call(y=y, il=il, lm=lm, **kw):
        return F.ctc_beam_search_decode_lm(y, il, lm, **kw)

    for name, fn in (('ctc_beam_search_decode', lambda **kw: F.ctc_beam_search_decode(y, il, **kw)),
                     ('ctc_beam_search_decode_lm', lm_call)):
        add(name + '_cpu', fn)
        add(name + '_beam_0', lambda fn=fn: fn(beam_width=0))
        add(name + '_beam_129', lambda fn=fn: fn(beam_width=129))
        add(name + '_paths_0', lambda fn=fn: fn(top_paths=0))
        add(name + '_paths_over_beam', lambda fn=fn: fn(beam_width=4, top_paths=5))
        add(name + '_beam_then_paths', lambda fn=fn: fn(beam_width=0, top_paths=0))
        add(name + '_paths_then_cpu', lambda fn=fn: fn(beam_width=200, top_paths=-3))
    add('ctc_beam_search_decode_lm_paths_then_weight', lambda: lm_call(top_paths=0, lm_weight=-1.0))
    add('ctc_beam_search_decode_lm_weight_neg', lambda: lm_call(lm_weight=-0.5))
    add('ctc_beam_search_decode_lm_weight_nan', lambda: lm_call(lm_weight=NAN))
    add('ctc_beam_search_decode_lm_weight_inf', lambda: lm_call(lm_weight=INF))
    add('ctc_beam_search_decode_lm_weight_then_bonus', lambda: lm_call(lm_weight=-1.0, insertion_bonus=INF))
    add('ctc_beam_search_decode_lm_bonus_inf', lambda: lm_call(insertion_bonus=-INF))
    add('ctc_beam_search_decode_lm_bonus_nan', lambda: lm_call(insertion_bonus=NAN))
    add('ctc_beam_search_decode_lm_bonus_then_order', lambda: lm_call(insertion_bonus=NAN, lm=types.SimpleNamespace(order=4, num_labels=4)))
    add('ctc_beam_search_decode_lm_order_0', lambda: lm_call(lm=types.SimpleNamespace(order=0, num_labels=4)))
    add('ctc_beam_search_decode_lm_order_4', lambda: lm_call(lm=types.SimpleNamespace(order=4, num_labels=4)))
    add('ctc_beam_search_decode_lm_order_then_labels', lambda: lm_call(lm=types.SimpleNamespace(order=4, num_labels=7)))
    add('ctc_beam_search_decode_lm_labels', lambda: lm_call(lm=types.SimpleNamespace(order=2, num_labels=5)))
    add('ctc_beam_search_decode_lm_labels_then_trigram',
        lambda: lm_call(y=torch.full((2, 8, 65), 0.01), lm=types.SimpleNamespace(order=3, num_labels=60)))
    add('ctc_beam_search_decode_lm_trigram_65', lambda: lm_call(y=torch.full((2, 8, 65), 0.01), lm=types.SimpleNamespace(order=3, num_labels=64)))
    add('ctc_beam_search_decode_lm_trigram_64_then_cpu',
        lambda: lm_call(y=torch.full((2, 8, 64), 0.01), lm=types.SimpleNamespace(order=3, num_labels=63)))
    add('ctc_beam_search_decode_lm_shape_then_cpu', lambda: lm_call(y=y[0]))

    def align(y=y, lab=lab, il=il, ll=ll):
        return F.ctc_forced_align(y, lab, il, ll)

    add('ctc_forced_align_cpu', align)
    add('ctc_forced_align_rank', lambda: align(y=y[0]))
    add('ctc_forced_align_empty', lambda: align(y=y[:, :0]))
    add('ctc_forced_align_classes_1', lambda: align(y=y[:, :, :1]))
    add('ctc_forced_align_classes_257', lambda: align(y=torch.full((2, 8, 257), 0.01)))
    add('ctc_forced_align_classes_then_labels', lambda: align(y=y[:, :, :1], lab=lab[0]))
    add('ctc_forced_align_labels_rank', lambda: align(lab=lab[0]))
    add('ctc_forced_align_labels_batch', lambda: align(lab=lab[:1]))
    add('ctc_forced_align_labels_list', lambda: align(lab=[[0, 1, 2]]))
    add('ctc_forced_align_labels_128', lambda: align(lab=torch.zeros((2, 128), dtype=torch.int64)))
    add('ctc_forced_align_labels_then_input_length', lambda: align(lab=torch.zeros((2, 128), dtype=torch.int64), il=torch.tensor([8])))
    add('ctc_forced_align_input_length_count', lambda: align(il=torch.tensor([8, 6, 4])))
    add('ctc_forced_align_input_length_columns', lambda: align(il=torch.tensor([[8, 6]])))
    add('ctc_forced_align_input_length_rank', lambda: align(il=torch.tensor([[[8], [6]]])))
    add('ctc_forced_align_input_length_list', lambda: align(il=[8]))
    add('ctc_forced_align_input_then_label_length', lambda: align(il=torch.tensor([8]), ll=torch.tensor([3])))
    add('ctc_forced_align_label_length_count', lambda: align(ll=torch.tensor([3])))
    add('ctc_forced_align_label_length_then_cpu', lambda: align(ll=torch.tensor([[3, 2]])))
    add('ctc_forced_align_column_lengths_then_cpu', lambda: align(il=torch.tensor([[8], [6]]), ll=torch.tensor([[3], [2]])))

    add('edit_distance_cpu', lambda: F.edit_distance(hyp, hl, ref, rl))
    add('edit_distance_list', lambda: F.edit_distance([[1, 2]], [2], [[1]], [1]))
    add('edit_distance_cpu_then_shape', lambda: F.edit_distance(hyp[0], hl, ref, rl))
    add('edit_distance_cpu_then_class_map', lambda: F.edit_distance(hyp, hl, ref, rl, class_map=[]))

    def ali(hyp=hyp, ref=ref, **kw):
        return F.edit_alignment(hyp, hl, ref, rl, **kw)

    add('edit_alignment_cpu', ali)
    add('edit_alignment_batches', lambda: ali(ref=ref[:1]))
    add('edit_alignment_hyp_1025', lambda: ali(hyp=torch.zeros((2, 1025), dtype=torch.int64)))
    add('edit_alignment_ref_1025', lambda: ali(ref=torch.zeros((2, 1025), dtype=torch.int64)))
    add('edit_alignment_batches_then_length', lambda: ali(hyp=torch.zeros((3, 1025), dtype=torch.int64)))
    add('edit_alignment_length_then_confusion', lambda: ali(ref=torch.zeros((2, 1025), dtype=torch.int64), confusion=conf[0]))
    add('edit_alignment_confusion_rank', lambda: ali(confusion=conf[0]))
    add('edit_alignment_confusion_not_square', lambda: ali(confusion=conf[:4].contiguous()))
    add('edit_alignment_confusion_empty', lambda: ali(confusion=conf[:0, :0]))
    add('edit_alignment_confusion_dtype', lambda: ali(confusion=conf.long()))
    add('edit_alignment_confusion_strided', lambda: ali(confusion=torch.zeros((5, 10), dtype=torch.int32)[:, ::2]))
    add('edit_alignment_confusion_list', lambda: ali(confusion=[[0]]))
    add('edit_alignment_confusion_258', lambda: ali(confusion=torch.zeros((258, 258), dtype=torch.int32)))
    add('edit_alignment_confusion_257_then_cpu', lambda: ali(confusion=torch.zeros((257, 257), dtype=torch.int32)))
    add('edit_alignment_confusion_then_cpu', lambda: ali(confusion=conf, class_map=[]))
    add('edit_alignment_rank_then_cpu', lambda: ali(hyp=hyp[0]))
    add('edit_alignment_list', lambda: F.edit_alignment([[1, 2]], [2], [[1]], [1]))

    for t, c, lmax in ((200, 62, 60), (200, 256, 127), (200, 257, 127), (200, 256, 128), (15236, 62, 127), (15237, 62, 127),
                       (16372, 2, 0), (16373, 2, 0), (1, 2, 0)):
        add('ctc_shape_supported_%d_%d_%d' % (t, c, lmax), lambda s=(t, c, lmax): F.ctc_shape_supported(*s))
    add('ctc_supported_cpu', lambda: F.ctc_supported(y, lab))
    add('ctc_supported_cpu_rank', lambda: F.ctc_supported(y[0], lab))
    add('ctc_supported_cpu_labels_rank', lambda: F.ctc_supported(y, lab[0]))
    add('ctc_supported_cpu_int', lambda: F.ctc_supported(y.long(), lab))
    assert len({c[0] for c in cases}) == len(cases)
    return cases


def _run_py(fn):
    try:
        return fn()
    except Exception as e:          # noqa: BLE001 -- the type is what gets recorded
        return [type(e).__name__, str(e)]


@pytest.fixture(scope='module')
def recorded():
    with open(os.path.join(GOLDEN, 'g20_ctc_errors.json')) as f:
        return json.load(f)


def test_the_tables_are_the_recorded_ones(recorded):
    assert sorted(recorded['c']) == sorted(c[0] for c in _c_cases())
    assert sorted(recorded['python']) == sorted(c[0] for c in _py_cases())


@pytest.mark.parametrize('buffers', [False, True], ids=['no_buffers', 'made_up_buffers'])
def test_codes_and_messages_are_the_recorded_ones(recorded, buffers):
    if buffers and torch.cuda.is_available():
        pytest.skip('made-up addresses are only passed where no kernel can run')
    got = {name: _run(fn) for name, with_buffers, fn in _c_cases() if with_buffers == buffers}
    assert got
    wrong = {name: (got[name], recorded['c'][name]) for name in got if got[name] != recorded['c'][name]}
    assert not wrong, wrong


def test_the_wrappers_refuse_as_recorded(recorded):
    got = {name: _run_py(fn) for name, fn in _py_cases()}
    wrong = {name: (got[name], recorded['python'][name]) for name in got if got[name] != recorded['python'][name]}
    assert not wrong, wrong


def test_every_kind_of_rejection_is_in_the_table(recorded):
    """The recorded table covers what it claims to: each status code, every entry point, the pairs that pin the order, and every
    wrapper with at least one refusal."""
    c = recorded['c']
    assert {L.QK_ERR_INVALID_ARG, L.QK_ERR_UNSUPPORTED, L.QK_ERR_WORKSPACE, 0} <= {rc for rc, _ in c.values()}
    assert not any(rc == L.QK_ERR_LAUNCH for rc, _ in c.values()), 'no case reaches a launch'
    for e in list(ENTRIES) + ['qk_ctc_workspace_bytes', 'qk_ctc_beam_workspace_bytes', 'qk_edit_align_workspace_bytes',
                              'qk_ctc_align_workspace_bytes']:
        assert sum(1 for name in c if name.startswith(e + '_') and '_then_' in name) >= 2 or e.endswith('_workspace_bytes'), e
        assert any(name.startswith(e + '_') for name in c), e
    # the launchers' own codes for a dtype no entry point checked, and the entry point that checks it itself
    assert c['qk_ctc_batch_cost_dtype_3'][0] == L.QK_ERR_INVALID_ARG and c['qk_ctc_batch_cost_limits_then_dtype'][0] == L.QK_ERR_UNSUPPORTED
    assert c['qk_ctc_forced_align_unsupported_dtype_3'][0] == L.QK_ERR_UNSUPPORTED
    py = recorded['python']
    for fn in ('ctc_batch_cost', 'ctc_cost_and_grad', 'ctc_greedy_decode', 'ctc_beam_search_decode', 'ctc_beam_search_decode_lm',
               'ctc_forced_align', 'edit_distance', 'edit_alignment'):
        assert any(name.startswith(fn + '_') and isinstance(v, list) for name, v in py.items()), fn
    assert {v[0] for v in py.values() if isinstance(v, list)} >= {'RuntimeError', 'ValueError'}
    assert {True, False} <= {v for name, v in py.items() if name.startswith('ctc_shape_supported_')}
