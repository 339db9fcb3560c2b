"""The register engine's LDS block after its round-10 repacking (csrc/mt_reg_lds.h): the per-id text
lengths are 16 bits wide from the 512 class up (a segment that fills a whole 64 KiB arena half is
remembered apart), the load's leaf marks pass through them, and the store of those classes reads the
property sets into registers before its staging words take their place; the 576 class runs four waves
per SIMD.  Documents of 500+ segments with props go through the plain kernels, the C64 form (clients
past 32) and the event-recording form; the whole-arena and insert-heavy documents through the small
classes, which keep the older block.  Bit-exact against the CPU oracle at launch sizes 1 (a store and
a reload after every op), 7 and 32.
Run on the GPU box: python -m pytest tests -m gpu"""
import functools

import pytest

pytestmark = pytest.mark.gpu

INSERT, REMOVE = 0, 1
MT_DERR_TEXT_ARENA = 5
ARENA = 64 * 1024
LAUNCHES = [1, 7, 32]
WHOLE = ''.join(chr(97 + (i * 7 + i // 26) % 26) for i in range(ARENA))  # no two windows of it alike nearby


def _engine(n, b):
    from fluidframework_amd.engine import MergeEngine
    return MergeEngine(n, text_capacity=ARENA, ops_per_launch=b)


@pytest.mark.parametrize('b', [1, 32])
def test_a_segment_that_fills_the_arena_survives_a_compaction(b):
    """One insert of 65536 characters, then an insert in front of it (no boundary split: the segment
    stays whole) that the arena has no room for: the engine compacts (the whole text moves to the other
    arena half), finds no room and halts the document before that message -- with its text intact."""
    from fluidframework_amd.oplog import build_batch
    batch = build_batch([[(1, 0, 0, 1, INSERT, 0, 0, WHOLE, None, 0),
                          (2, 1, 1, 2, INSERT, 0, 0, 'x', None, 0)]])
    eng = _engine(1, b)
    eng.apply(batch)
    assert eng.error(0) == (MT_DERR_TEXT_ARENA, 2)
    assert eng.text(0) == WHOLE
    assert [s[0] for s in eng.state(0)['segs']] == [WHOLE]


@functools.lru_cache(maxsize=None)
def _cut_case():
    """the whole-arena segment cut twice by a remove, the tombstone unlinked once the msn passes it, then
    an insert that fits only after a compaction"""
    from fluidframework_amd.oplog import build_batch
    from oracle import oracle
    oracle.build()
    batch = build_batch([[(1, 0, 0, 1, INSERT, 0, 0, WHOLE, None, 0),
                          (2, 1, 1, 2, REMOVE, 1000, 2000, None, None, 0),
                          (3, 2, 2, 1, REMOVE, 0, 1, None, None, 0),
                          # (the msn reaches 3 before the insert: the block's LRU entry of seq 3 is popped and
                          # both tombstones are unlinked, so the compaction that the insert needs frees their
                          # text.  Every acked piece next to another is longer than TextSegmentGranularity, so
                          # zamboni appends none: an append's copy would need arena room of its own)
                          (4, 3, 3, 2, REMOVE, 3000, 3001, None, None, 0),
                          (5, 4, 4, 2, INSERT, 5, 0, 'y' * 50, {1: 3}, 0),
                          (6, 5, 5, 1, INSERT, 60000, 0, 'zz\n', None, 0)]])
    o = oracle.Oracle(1).apply(batch, threads=1)
    assert o.error(0) == (0, 0)
    return batch, o


@pytest.mark.parametrize('b', LAUNCHES)
def test_cut_whole_arena_segment_against_oracle(b):
    batch, o = _cut_case()
    eng = _engine(1, b)
    eng.apply(batch)
    assert eng.error(0) == (0, 0)
    assert int(eng.checksums()[0]) == int(o.checksums()[0])
    assert eng.state(0) == o.state(0)
    assert eng.text(0) == o.text(0)


N_DOCS = 64


@functools.lru_cache(maxsize=None)
def _synth():
    """64 documents x 160 ops of C3's mix with p_insert = 0.8 (inserts inside segments, with and without
    props, between removes and annotates); the oracle replays every one without an error"""
    from fluidframework_amd.oplog import CONFIGS
    from oracle import oracle
    oracle.build()
    cfg = dict(CONFIGS['C3'], ops_per_doc=160, p_insert=0.8, p_remove=0.15, max_lag=32)
    cfg.pop('n_docs')
    batch = oracle.generate(N_DOCS, seed=1010, **cfg)
    o = oracle.Oracle(N_DOCS).apply(batch, threads=4)
    for d in range(N_DOCS):
        assert o.error(d) == (0, 0), (d, o.error(d))
    return batch, o


@pytest.mark.parametrize('b', LAUNCHES)
def test_insert_heavy_documents_against_oracle(b):
    batch, o = _synth()
    eng = _engine(N_DOCS, b)
    eng.apply(batch)
    cs, want = eng.checksums(), o.checksums()
    for d in range(N_DOCS):
        assert eng.error(d) == (0, 0), (d, eng.error(d))
        assert int(cs[d]) == int(want[d]), d
        assert eng.state(d) == o.state(d), d


# ---- documents of 500+ segments: the classes from 512 slots up (K >= 8), whose store stages through
# props' words, in the three kernel forms
N_BIG = 12
FORMS = {'plain': 32, 'c64': 48, 'ev': 32}  # form -> clients (ids past 32 take the C64 form)
CLASS_FLAGS = 0xFC000000
MT_CLASS_C64 = 0x10000000


@functools.lru_cache(maxsize=None)
def _big(n_clients):
    """C3's mix (props on inserts and annotates, overlapping removes), 1024 ops per document"""
    from fluidframework_amd.oplog import CONFIGS
    from oracle import oracle
    oracle.build()
    cfg = dict(CONFIGS['C3'], n_clients=n_clients)
    cfg.pop('n_docs')
    batch = oracle.generate(N_BIG, seed=1012, **cfg)
    o = oracle.Oracle(N_BIG).record_events().apply(batch, threads=4)
    for d in range(N_BIG):
        assert o.error(d) == (0, 0), (d, o.error(d))
    sizes = [len(o.state(d)['segs']) for d in range(N_BIG)]
    assert max(sizes) >= 500 and any(s[6] for d in range(0, N_BIG, 5) for s in o.state(d)['segs']), sizes
    return batch, o


@pytest.mark.parametrize('b', LAUNCHES)
@pytest.mark.parametrize('form', sorted(FORMS))
def test_documents_of_500_segments_in_every_kernel_form(form, b):
    batch, o = _big(FORMS[form])
    if form == 'c64':
        assert int(batch.ops['client'].max()) > 32
    eng = _engine(N_BIG, b)
    if form == 'ev':
        eng.enable_events(1 << 16)
    assert eng.class_kernel(576).startswith('mtr::reg_apply_kernel')
    eng.apply(batch)
    # the launches ran in the register classes from 512 slots up, not on the LDS engine
    # (the C64 form reports its classes as MT_CLASS_C64 | capacity)
    used = {cap for cap, _, launches, _ in eng.last_class_stats() if launches}
    form_flag = MT_CLASS_C64 if form == 'c64' else 0
    assert any(512 <= cap & ~CLASS_FLAGS <= 1024 for cap in used if cap & CLASS_FLAGS == form_flag), sorted(used)
    cs, want = eng.checksums(), o.checksums()
    for d in range(N_BIG):
        assert eng.error(d) == (0, 0), (form, d, eng.error(d))
        assert int(cs[d]) == int(want[d]), (form, d)
        assert eng.state(d) == o.state(d), (form, d)
    if form == 'ev':
        got = eng.drain_events()
        for d in range(N_BIG):
            assert got[d] == o.events(d), (form, d)
