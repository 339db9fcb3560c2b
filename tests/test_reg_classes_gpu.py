"""Small and whole-arena documents in every class of the register engine (csrc/mt_apply_reg.hip): 15
capacity classes (K = 2 ... 16) times the plain, C64 (clients past 32) and event-recording kernels, each
its own instantiation.  mt_bin_kernel bins by the launch's worst-case growth, so the size of a launch --
a log's tail padded with non-op records, or ops_per_launch -- takes a small document to any class
(tests/reg_classes.py; test_reg_classes.py checks the inputs on the CPU).

A. a segment that fills the whole 64 KiB arena half, in the classes whose LDS block keeps text lengths in
   16 bits (K >= 8: the segment's length is 0 there and RLds::big remembers its id) and in K = 7, the
   last class with 32-bit lengths: the insert, the boundary split, zamboni's unlink, the load and
   compact_text each read or write `big`.
B. shrinking, annotate-heavy and churning documents of a few hundred records, and documents whose text
   turns over in a 2 KiB arena half (a compaction every ten cycles), through every class and form.
C. the error fixtures, whose documents halt in the middle of a launch, in the large classes.

Everything is bit-exact against the CPU oracle: error, checksum, state, text, and the callbacks in the
event-recording form.  Every apply asserts from last_class_stats() that its class ran, on the register
engine.  Run on the GPU box: python -m pytest tests -m gpu"""
import pytest

import reg_classes as rc
from reg_classes import ARENA, FORMS, K_ALL, K_ARENA, K_HALT, MT_DERR_TEXT_ARENA, launch_size

pytestmark = pytest.mark.gpu


def _engine(n_docs, form, ops_per_launch=0, text_capacity=ARENA, events=1 << 12):
    from fluidframework_amd.engine import MergeEngine
    eng = MergeEngine(n_docs, text_capacity=text_capacity, ops_per_launch=ops_per_launch)
    if form == 'ev':
        eng.enable_events(events)
    return eng


def _same(eng, o, form, where, events=None):
    """every document of the engine against the oracle's; `events` (ev form): the callbacks drained now"""
    cs, want = eng.checksums(), o.checksums()
    for d in range(eng.n_docs):
        assert eng.error(d) == o.error(d), (where, d, eng.error(d))
        assert int(cs[d]) == int(want[d]), (where, d)
        assert eng.state(d) == o.state(d), (where, d)
        assert eng.text(d) == o.text(d), (where, d)
        if form == 'ev':
            assert events[d] == o.events(d), (where, d)


# ---- A ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('name', sorted(rc.SCENARIOS))
def test_whole_arena_segment(name, form):
    shift = rc.C64_SHIFT if form == 'c64' else 0
    for K in K_ARENA:
        batches, o = rc.scenario(name, launch_size(K), shift)
        eng = _engine(1, form)
        for b in batches:  # (each apply one launch of launch_size(K) records)
            eng.apply(b)
            assert rc.used_classes(eng, form) == {K} and rc.no_lds_launches(eng), (name, K, rc.launched(eng))
        where = (name, form, K)
        events = eng.drain_events() if form == 'ev' else None
        if name == 'A1':
            # the oracle has no arena: it stands before the record the engine halts on
            assert eng.text(0) == rc.WHOLE and [s[0] for s in eng.state(0)['segs']] == [rc.WHOLE], where
            assert eng.error(0) == (MT_DERR_TEXT_ARENA, 2), where
            assert eng.state(0) == o.state(0) and int(eng.checksums()[0]) == int(o.checksums()[0]), where
            assert events is None or events[0] == o.events(0), where
        else:
            _same(eng, o, form, where, events)


# ---- B ----------------------------------------------------------------------------------------------
def _every_class(form, run):
    """run(step) -> the engine after the apply meant for `step` ('small': K = 2 ... 4 by segment count at
    32 records per launch; K = 5 ... 16 by launch size).  A document may go to the class above when its
    tree grows; a class never reached fails."""
    reached = set()
    for step in rc.B_STEPS:
        eng = run(step)
        used = rc.used_classes(eng, form)
        want = {2, 3, 4} if step == 'small' else {step}
        assert want <= used <= want | {max(want) + 1} and rc.no_lds_launches(eng), (form, step, rc.launched(eng))
        reached |= used
    assert set(K_ALL) <= reached, (form, sorted(reached))


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('name', sorted(rc.WORKLOADS))
def test_small_documents_in_every_class(name, form):
    def run(step):
        clients = rc.n_clients(name, form)
        batch, o, _ = rc.workload(name, clients, step)
        cap = rc.churn_arena(clients, step)[0] if name == 'churn' else ARENA
        eng = _engine(rc.N_DOCS, form, rc.step_launch(step), cap)
        eng.apply(batch)
        _same(eng, o, form, (name, form, step), eng.drain_events() if form == 'ev' else None)
        return eng
    _every_class(form, run)


@pytest.mark.parametrize('form', FORMS)
def test_tight_arenas_compact_in_every_class(form):
    """three launches of 8 K records per document: a new document, then two loads of a stored one, with
    some 7 (K = 5) to 23 (K = 16) arena halves of text written through each"""
    shift = rc.C64_SHIFT if form == 'c64' else 0
    for K in range(5, 17):
        batch, o, _ = rc.turnover(K, shift)
        eng = _engine(rc.N_DOCS, form, launch_size(K), rc.TURN_ARENA)
        eng.apply(batch)
        assert rc.used_classes(eng, form) == {K} and rc.no_lds_launches(eng), (form, K, rc.launched(eng))
        _same(eng, o, form, ('turnover', form, K), eng.drain_events() if form == 'ev' else None)


# ---- C ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('form', ['plain', 'ev'])
@pytest.mark.parametrize('fixture', rc.HALT_FIXTURES)
def test_halts_in_the_large_classes(fixture, form):
    """the store after a halt in the middle of a launch (K >= 8: its staging takes the place of the
    property words) and mt_fixup_kernel's precedence, with launches of up to 128 records"""
    from test_errors import ref_code
    for K in K_HALT:
        batch, o, exp = rc.halts(fixture, K)
        eng = _engine(batch.n_docs, form)
        eng.apply(batch)
        assert rc.used_classes(eng, form) == {K} and rc.no_lds_launches(eng), (fixture, K, rc.launched(eng))
        _same(eng, o, form, (fixture, form, K), eng.drain_events() if form == 'ev' else None)
        cs = eng.checksums()
        halted = 0
        for r in exp:  # a halted document ignores the padding: the reference's own record of it
            d, code = r['doc'], ref_code(r['err'])
            if code:
                halted += 1
                assert eng.error(d) == (code, r['err_seq']), (fixture, form, K, d)
                assert eng.state(d) == r['state'] and '%016x' % cs[d] == r['checksum'], (fixture, form, K, d)
        assert halted
