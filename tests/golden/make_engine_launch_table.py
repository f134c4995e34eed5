"""What the library DECIDES about a call, as the PARENT commit's library decides it -> tests/golden/engine_launch_table.json:
the verdict of smart_check_ensemble, smart_workspace_bytes and the text of smart_describe_launch for some 230 calls that
between them reach every branch of check(), merged_report(), plan_time_slices(), decide(), illcond_form(), layout()
and carve() (smart_capi.hip).  Nothing is allocated and nothing is launched: the pointers of a row are dummies.

Recorded in two passes, each with the parent's library selected (the file of the first pass is completed by the second):

    bash tools/build_rev_variant.sh <parent rev> parent
    export SMART_AMD_LIB=$PWD/tools/variants/libsmart_amd_parent.so
    python tests/golden/make_engine_launch_table.py [out.json]      # without a device: check, bytes_no_device
    python tests/golden/make_engine_launch_table.py [out.json]      # on an MI355X: bytes_device, describe

The change the fixture was made for rewrote how the C side keeps its kernel table, its workspace layout and its
environment overrides, and no decision.  The rows and how a row becomes a call live here, so that
tests/test_launch_table.py asks exactly what the fixture recorded.

A row: `e` the integer and float fields of SmartEnsemble that differ from BASE, `pointers` the fields that hold the
dummy address, `workspace` what the call's workspace is ("none": NULL; "full": as many bytes as smart_workspace_bytes
asks for; a number: that many bytes), `env` the overrides set around the calls.
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'engine_launch_table.json')
OVERRIDES = ('SMART_TIME_SLICES', 'SMART_EXITS', 'SMART_ILLCOND_FORM')
REQUIRED = ('area_m2', 'forcing', 'params', 'gw')
T = 24 * 3653                    # ten years of hourly steps: a multiple of 24, 8, 6 and 2
BASE = dict(n_catchments=1, n_samples=100000, n_steps=T, n_warm=0, report_gap=24, report_type=1, math_mode=1,
            delta_sec=3600.0)
VALID, REGULAR, STIFF, GUARD, ILLCOND = 0x100, 0x01, 0x02, 0x04, 0x08
PIECEWISE, VARYING, ORDERED, RUNS = 0x10, 0x20, 0x40, 0x80
COUNT_SHIFT, COUNT_MAX = 12, 0x7ffff
N_SIMD = 1024                    # of the MI355X the device columns were recorded on (256 CUs)


def n_reports(e):
    gap = e['report_gap']
    return (e['n_steps'] + gap - 1) // gap if e['report_type'] == 2 else e['n_steps'] // gap


def blocks_of(e):
    return (e['n_samples'] + 63) // 64 * e['n_catchments']


def room(e, objfn, handover=False, extra=0):
    """bytes of a workspace that ends behind the observation statistics, or behind the hand-over of a sliced launch"""
    n = ((64 + e['n_catchments']) * 4 + 255) // 256 * 256
    if objfn:
        n += e['n_catchments'] * (8 + n_reports(e)) * 8
    if handover:
        n += blocks_of(e) * 23 * 64 * 8 + (blocks_of(e) + 1) // 2 * 2 * 4
    return n + extra


def rows():
    out = []

    def add(name, workspace='full', pointers=(), env=None, drop=(), **fields):
        e = dict(BASE, **fields)
        ptrs = [p for p in REQUIRED if p not in drop] + list(pointers)
        if 'objfn' in ptrs and 'obs' not in ptrs and 'obs' not in drop:
            ptrs.append('obs')
        if callable(workspace):
            workspace = workspace(e, 'objfn' in ptrs)
        out.append(dict(name=name, e={k: v for k, v in e.items() if BASE.get(k) != v}, pointers=sorted(set(ptrs)),
                        workspace=workspace, env=dict(env or {})))

    # ---- every refusal of check(), in its order (a NULL SmartEnsemble: the test asks that one itself)
    add('ok')
    for f in ('n_catchments', 'n_samples', 'n_steps', 'report_gap'):
        add('refuse_%s_0' % f, **{f: 0})
    add('refuse_n_warm_negative', n_warm=-24)
    add('refuse_report_type_3', report_type=3)
    add('refuse_report_type_0', report_type=0)
    add('refuse_math_mode_5', math_mode=5)
    add('refuse_math_mode_negative', math_mode=-1)
    add('refuse_warm_beyond_run', n_warm=T + 24)
    add('warm_equals_run', n_warm=T)
    add('refuse_summary_length_ragged', n_steps=T + 1)
    add('refuse_summary_warm_ragged', n_warm=12)
    add('raw_tolerates_ragged_warm', report_type=2, n_warm=12)
    add('refuse_delta_sec_0', delta_sec=0.0)
    add('refuse_delta_sec_negative', delta_sec=-1.0)
    add('refuse_delta_sec_nan', delta_sec='nan')          # (as text: a NaN has no place in a JSON file)
    for p in REQUIRED:
        add('refuse_no_%s' % p, drop=(p,))
    add('refuse_params_stride_short', params_catchment_stride=10 * 100000 - 1)
    add('params_stride_exact', params_catchment_stride=10 * 100000)
    add('refuse_discharge_ld_short', pointers=('discharge',), discharge_ld=99999)
    add('discharge_ld_exact', pointers=('discharge',), discharge_ld=100000)
    add('refuse_objfn_without_obs', pointers=('objfn',), drop=('obs',))
    add('refuse_objfn_without_workspace', pointers=('objfn',), workspace='none')
    add('refuse_workspace_short_of_statistics', pointers=('objfn',), workspace=lambda e, o: room(e, o) - 8)
    add('refuse_time_slices_negative', time_slices=-1)
    add('refuse_plan_without_valid_bit', plan=REGULAR | PIECEWISE)
    add('refuse_literal_form_3', literal_form=3)
    add('refuse_literal_form_negative', literal_form=-1)

    # ---- report shapes: merged_report(), uses_records(), layout(); with and without final_vars and objfn
    shapes = [('summary', 1, g, T) for g in (24, 8, 6, 2, 1)] + [('raw', 2, g, T) for g in (24, 6, 1)] + \
             [('raw_ragged', 2, 24, T + 1), ('raw_ragged', 2, 6, T + 1)]
    for kind, rtype, gap, steps in shapes:
        for final in (False, True):
            for objfn in (False, True):
                ptrs = (('final_vars',) if final else ()) + (('objfn',) if objfn else ())
                add('%s_gap%d%s%s' % (kind, gap, '_final' if final else '', '_objfn' if objfn else ''), pointers=ptrs,
                    report_type=rtype, report_gap=gap, n_steps=steps)
    add('raw_gap24_ragged_warm', report_type=2, n_warm=12)
    add('summary_gap24_warm', n_warm=24 * 365)
    for kind, rtype, gap in (('summary', 1, 24), ('summary', 1, 6), ('raw', 2, 24), ('raw', 2, 1)):
        add('literal_%s_gap%d' % (kind, gap), math_mode=0, report_type=rtype, report_gap=gap)
        add('literal_%s_gap%d_objfn' % (kind, gap), math_mode=0, report_type=rtype, report_gap=gap, pointers=('objfn',))

    # ---- n_samples x n_catchments on both sides of each threshold of plan_time_slices() and of the early exits
    for name, n in (('one_block_per_simd', 65536), ('one_block_per_simd_plus', 65600), ('load_2_5', 163840),
                    ('load_2_5_plus', 163904), ('ten_per_simd_minus', 655296), ('ten_per_simd', 655360),
                    ('48_per_simd', 3145728), ('48_per_simd_plus', 3145792), ('one_sample', 1), ('one_block', 64),
                    ('one_block_plus', 65)):
        add('size_%s' % name, n_samples=n)
        add('size_%s_objfn_raw' % name, n_samples=n, report_type=2, pointers=('objfn', 'discharge'), discharge_ld=n)
    add('size_64_catchments', n_catchments=64, n_samples=10000)
    add('size_64_catchments_objfn', n_catchments=64, n_samples=10000, pointers=('objfn',))
    add('size_64_catchments_gap1', n_catchments=64, n_samples=10000, report_gap=1)
    add('size_1025_catchments_of_one_block', n_catchments=1025, n_samples=64)

    # ---- short runs: n_all < 64, n_all / 64 < 24 (and the warm-up counts)
    for days in (63, 64, 127, 640, 24 * 64 - 1, 24 * 64):
        add('short_%d_days' % days, n_steps=24 * days)
    add('short_40_days_24_warm', n_steps=24 * 40, n_warm=24 * 24)
    add('short_40_days_23_warm', n_steps=24 * 40, n_warm=24 * 23)
    add('short_63_steps_gap1', n_steps=63, report_gap=1)
    add('short_64_steps_gap1', n_steps=64, report_gap=1)

    # ---- time_slices and SMART_TIME_SLICES
    for ts in (0, 1, 2, 5, 913, 1000):
        add('time_slices_%d' % ts, time_slices=ts)
    add('time_slices_5_small_launch', time_slices=5, n_samples=640)
    add('time_slices_5_huge_launch', time_slices=5, n_samples=3145792)
    add('time_slices_5_short_run', time_slices=5, n_steps=24 * 63)
    add('time_slices_30_of_100_days', time_slices=30, n_steps=24 * 100)
    add('time_slices_5_plain_kernel', time_slices=5, report_type=2, n_steps=T + 1)
    for v in ('0', '1', '-3', '8', '5000', 'x'):
        add('env_time_slices_%s' % v, env={'SMART_TIME_SLICES': v})
    add('env_time_slices_8_field_5', env={'SMART_TIME_SLICES': '8'}, time_slices=5)
    add('env_time_slices_8_field_1', env={'SMART_TIME_SLICES': '8'}, time_slices=1)
    add('env_time_slices_8_small_launch', env={'SMART_TIME_SLICES': '8'}, n_samples=640)

    # ---- workspace room: carve()
    add('workspace_none', workspace='none')
    add('workspace_none_raw', workspace='none', report_type=2)
    add('workspace_short_of_header', workspace=100)
    add('workspace_header_only', workspace=lambda e, o: room(e, o))
    add('workspace_statistics_only', pointers=('objfn',), workspace=lambda e, o: room(e, o))
    add('workspace_short_of_handover', pointers=('objfn',), workspace=lambda e, o: room(e, o, True, -8))
    add('workspace_handover_no_codes', pointers=('objfn',), workspace=lambda e, o: room(e, o, True))
    # (the code words of this call: 8 bytes per chunk of four steps and four chunks more, rounded up to 256)
    add('workspace_handover_short_of_codes', workspace=lambda e, o: room(e, o, True, ((T // 4 + 4) * 8 + 255) // 256 * 256 - 8))
    add('workspace_handover_no_records_gap1', report_gap=1, workspace=lambda e, o: room(e, o, True))
    add('workspace_more_than_asked', workspace=lambda e, o: room(e, o, True, 1 << 24))
    add('workspace_codes_unsliced', n_samples=640, workspace=lambda e, o: room(e, o, False, 1 << 20))
    add('workspace_header_only_unsliced', n_samples=640, workspace=lambda e, o: room(e, o))

    # ---- the plan: decide()
    add('plan_0', plan=0)
    for name, bit in (('regular', REGULAR), ('stiff', STIFF), ('guard', GUARD), ('illcond', ILLCOND),
                      ('piecewise', PIECEWISE), ('varying', VARYING), ('runs', RUNS), ('ordered', ORDERED)):
        add('plan_%s_alone' % name, plan=VALID | bit)
    add('plan_valid_alone', plan=VALID)
    for kind, fields in (('summary', {}), ('summary_final', {}), ('raw', dict(report_type=2)),
                         ('every', dict(report_gap=1)), ('plain', dict(report_type=2, n_steps=T + 1))):
        ptrs = ('final_vars',) if kind == 'summary_final' else ()
        for name, bits in (('piecewise', PIECEWISE), ('varying', VARYING), ('runs', RUNS),
                           ('runs_varying', RUNS | VARYING), ('all_forcing', PIECEWISE | VARYING | RUNS)):
            add('plan_%s_regular_%s' % (kind, name), plan=VALID | REGULAR | bits, pointers=ptrs, **fields)
    add('plan_all_bits', plan=VALID | 0xff | (7 << COUNT_SHIFT))
    add('plan_all_bits_saturated', plan=VALID | 0xff | (COUNT_MAX << COUNT_SHIFT))
    add('plan_all_classes_piecewise_exits', plan=VALID | 0xf | PIECEWISE, n_samples=163904)
    add('plan_all_classes_runs_exits', plan=VALID | 0xf | RUNS, n_samples=163904)
    add('plan_all_classes_runs_no_exits', plan=VALID | 0xf | RUNS, n_samples=163840)
    # class-3 blocks on both sides of blocks * 16 + (all - blocks) <= 2 * n_simd: 30,000 samples are 469 blocks
    for count in (1, 105, 106, 469, COUNT_MAX - 1, COUNT_MAX):
        add('plan_illcond_count_%d' % count, n_samples=30000, plan=VALID | 0xf | PIECEWISE | (count << COUNT_SHIFT))
    add('plan_illcond_no_count', n_samples=30000, plan=VALID | 0xf | PIECEWISE)
    add('plan_illcond_saturated_few_blocks', n_samples=6400, plan=VALID | 0xf | PIECEWISE | (COUNT_MAX << COUNT_SHIFT))
    add('plan_illcond_alone_counted', n_samples=30000, plan=VALID | ILLCOND | (105 << COUNT_SHIFT))
    add('plan_0_few_blocks', n_samples=6400, plan=0)
    add('plan_0_128_blocks', n_samples=8192, plan=0)
    add('plan_0_129_blocks', n_samples=8256, plan=0)

    # ---- literal_form and the overrides of the environment
    for form in (0, 1, 2):
        add('literal_form_%d_few' % form, literal_form=form, n_samples=6400)
        add('literal_form_%d_many' % form, literal_form=form)
        for v in ('rows', 'lanes'):
            add('literal_form_%d_env_%s' % (form, v), literal_form=form, env={'SMART_ILLCOND_FORM': v})
    add('env_illcond_form_rows_few', n_samples=6400, env={'SMART_ILLCOND_FORM': 'rows'})
    add('env_illcond_form_lanes_few', n_samples=6400, env={'SMART_ILLCOND_FORM': 'lanes'})
    add('env_illcond_form_other', env={'SMART_ILLCOND_FORM': 'auto'})
    for v in ('0', '1', 'x'):
        for name, n in (('load_2_5', 163840), ('load_2_5_plus', 163904)):
            add('env_exits_%s_%s' % (v, name), n_samples=n, env={'SMART_EXITS': v})
    add('env_exits_1_final', env={'SMART_EXITS': '1'}, pointers=('final_vars',))
    add('env_exits_0_runs', env={'SMART_EXITS': '0'}, n_samples=163904, plan=VALID | REGULAR | RUNS)
    add('env_all_three', env={'SMART_EXITS': '1', 'SMART_TIME_SLICES': '4', 'SMART_ILLCOND_FORM': 'lanes'}, n_samples=6400)
    assert len({r['name'] for r in out}) == len(out)
    return out


def ensemble(row, address, workspace_bytes=0):
    """the SmartEnsemble of a row; `address`: what its pointers hold"""
    from smartpy_amd import _lib
    e = _lib.SmartEnsemble()
    for k, v in dict(BASE, **row['e']).items():
        setattr(e, k, float(v) if k == 'delta_sec' else v)
    for p in row['pointers']:
        setattr(e, p, address)
    if row['workspace'] != 'none':
        e.workspace = address
        e.workspace_bytes = workspace_bytes if row['workspace'] == 'full' else row['workspace']
    return e


def ask(L, row, address, with_device):
    """what the library says about a row: {'check': [rc, text], 'bytes': n} and, with a device, 'describe': [rc, text,
    error text]"""
    before = {k: os.environ.pop(k, None) for k in OVERRIDES}
    try:
        os.environ.update(row['env'])
        need = L.smart_workspace_bytes(ctypes.byref(ensemble(row, address)))
        e = ensemble(row, address, need)
        got = {'bytes': need, 'bytes_with_workspace': L.smart_workspace_bytes(ctypes.byref(e))}
        got['check'] = [L.smart_check_ensemble(ctypes.byref(e)), L.smart_last_error().decode()]
        if with_device:
            text = ctypes.create_string_buffer(1024)
            rc = L.smart_describe_launch(ctypes.byref(e), text, len(text))
            got['describe'] = [rc, text.value.decode(), L.smart_last_error().decode() if rc else '']
    finally:
        for k in OVERRIDES:
            os.environ.pop(k, None)
            if before[k] is not None:
                os.environ[k] = before[k]
    return got


def device_cus(L):
    """CUs of the visible device, or 0"""
    if L.smart_device_count() < 1:
        return 0
    import torch
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def main(path):
    from smartpy_amd import _lib
    L = _lib.lib()
    print('library:', _lib.LIB_PATH)
    table = {'multi_processor_count': None, 'rows': rows()}
    if os.path.exists(FIXTURE):         # the other pass's columns stay
        old = json.load(open(FIXTURE))
        by_name = {r['name']: r for r in old['rows']}
        table['multi_processor_count'] = old['multi_processor_count']
        for r in table['rows']:
            o = by_name.get(r['name'])
            if o and all(o[k] == r[k] for k in ('e', 'pointers', 'workspace', 'env')):
                r.update({k: o[k] for k in ('check', 'bytes_no_device', 'bytes_device', 'describe') if k in o})
    cus = device_cus(L)
    buf = (ctypes.c_double * 16)()
    for r in table['rows']:
        got = ask(L, r, ctypes.addressof(buf), cus > 0)
        assert got['bytes_with_workspace'] == got['bytes'], r['name']
        if cus:
            assert r.get('check', got['check']) == got['check'], r['name']
            r['bytes_device'], r['describe'] = got['bytes'], got['describe']
        else:
            r['check'], r['bytes_no_device'] = got['check'], got['bytes']
    if cus:
        table['multi_processor_count'] = cus
    with open(path, 'w') as f:
        f.write('{"multi_processor_count": %s,\n "rows": [\n' % json.dumps(table['multi_processor_count']))
        f.write(',\n'.join('  ' + json.dumps(r, sort_keys=True) for r in table['rows']))
        f.write('\n ]}\n')
    print('%d rows (%s) -> %s' % (len(table['rows']), '%d CUs' % cus if cus else 'no device', path))


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else FIXTURE)
