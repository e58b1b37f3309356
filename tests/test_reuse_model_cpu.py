"""The generator of the handle re-use test (tests/reuse_model.py) on the CPU, with a handle that only records its calls, over
the seeds the GPU test runs: the random sequences reach what they are for -- every setter, every compute kind in both forms,
both dtypes and homes of uo/vo, captured passes that a later op replays after tracer and class calls, every cause of
refusal -- and refusals stay a minority."""
import collections

import numpy

from reuse_model import (BOTH_FORMS, KINDS, NOPS, REFUSAL_CLASSES, SEEDS, SETTERS, Model, RecordingHandle, run_sequence)


def logs(seed):
    model, h = Model(numpy.random.default_rng(seed)), RecordingHandle()
    run_sequence(model, h, NOPS, lambda plan: None)
    return model.log, h.calls


def all_logs():
    out = []
    for seed in SEEDS:
        out += logs(seed)[0]
    return out


def computes(log):
    return [e[1] for e in log if e[0] == 'compute']


def test_every_setter_op_occurs():
    n = collections.Counter(e[1] for e in all_logs() if e[0] == 'set')
    print(sorted(n.items()))
    assert set(n) == set(SETTERS)
    for op in SETTERS:           # the four cell-thickness homes, both clearing ops and the three streams are among them
        assert n[op] >= 5, (op, n[op])


def test_every_compute_kind_succeeds_in_both_forms_dtypes_and_homes():
    plans = computes(all_logs())
    fine = [p for p in plans if not p['codes']]
    n = collections.Counter(p['kind'] for p in fine)
    print(sorted(n.items()))
    for kind in KINDS:
        assert n[kind] >= 5, (kind, n[kind])
    for kind in BOTH_FORMS:
        assert {p['form'] for p in plans if p['kind'] == kind} == {'sync', 'async'}, kind
    assert {p['dtype'] for p in fine} == {'float32', 'float64'}
    assert {p['uv_on_device'] for p in fine} == {False, True}


def test_graph_replays_are_reached():
    """Model.capturable() says when nf_field_compute_all_async captures its pass (non-null stream, resident uo / vo, resident
    thickness, not the all-steps-in-one-launch form); the second call of every such 'all' is a replay.  Some must come with a
    static HBM thickness, and some must replay a pass that an EARLIER op captured, with nothing but tracer / class setters
    and other computes in between, a tracer setter among them: "the setters do not invalidate a captured pass"."""
    fine = [p for p in computes(all_logs()) if p['kind'] == 'all' and not p['codes'] and p['stream'] != 0]
    assert any(p['ct_home'] == 'ct_static_hbm' for p in fine)
    assert any(p['tracer_set_after_all'] for p in fine)
    captured = [p for p in fine if p['capturable']]
    print(len(captured), 'captured passes,', sum(p['replay_after_others'] for p in captured), 'replayed by a later op')
    assert len(captured) >= 3
    assert any(p['ct_home'] == 'ct_static_hbm' for p in captured) and any(p['ct_home'] is None for p in captured)
    assert any(p['replay_after_others'] for p in captured)
    assert any(p['replay_after_others'] and p['tracer_set_after_all'] for p in captured)
    for p in computes(all_logs()):
        assert not p['capturable'] or (p['stream'] != 0 and p['uv_on_device'] and p['ct_home'] != 'ct_tv_host')


def test_every_refusal_class_is_reached_and_refusals_stay_a_minority():
    plans = computes(all_logs())
    refused = [p for p in plans if p['codes']]
    for name, causes in REFUSAL_CLASSES.items():
        n = sum(1 for p in refused if set(p['causes']) & set(causes))
        print(name, n)
        assert n >= 2, (name, n)
    print(len(refused), 'of', len(plans), 'computes are refused')
    assert len(refused) <= 0.4 * len(plans)
    for p in plans:              # a refusal names its codes, and only documented ones
        assert bool(p['causes']) == bool(p['codes']) and set(p['codes']) <= {1, 2}


def test_same_seed_same_sequence():
    def plain(x):
        if isinstance(x, numpy.ndarray):
            return (x.shape, x.dtype.name, x.tobytes())
        if isinstance(x, (tuple, list)):
            return tuple(plain(y) for y in x)
        return repr(x) if isinstance(x, float) else x

    for seed in SEEDS[:4]:
        (log_a, calls_a), (log_b, calls_b) = logs(seed), logs(seed)
        assert log_a == log_b
        assert plain(calls_a) == plain(calls_b)
    assert logs(SEEDS[0])[0] != logs(SEEDS[1])[0]
