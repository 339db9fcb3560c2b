"""An editing client on a wide document, on the device (mt_apply.hip: apply_kernel_g<CAP, W, LOC, GW>, the
wide editing form; include/mtgpu.h "limits"): UTF-16 text, keys 0..31, u16 value ids, client ids up to
65534 -- the editing client's own included -- with edits pending.

Pinned by the reference itself: tests/golden/localw_*.expected.jsonl hold the canonical states of the
reference's editing client at checkpoints and at the end, as checksums (tests/golden/make_localw.py;
localw.same_state compares).  The CPU oracle
refuses editing-and-wide documents, so nothing here compares with it.  Before this form the engine halted
such a document with MT_DERR_LIMITS at its first wide record."""
import hashlib
import json

import numpy as np
import pytest

import localw
from localw import CLASS_EDITING, CLASS_GROUPS, CLASS_WIDE, LOGS, LONG

pytestmark = pytest.mark.gpu
MT_DERR_CAPACITY, MT_DERR_LIMITS = 4, 6


def used_classes(eng):
    return {cap for cap, _, launches, _ in eng.last_class_stats() if launches}


def run_steps(name, b, check, events=False, **kw):
    """Apply the log checkpoint by checkpoint on one engine (the launches of a step carry b records per
    document); check(eng, q, rows, classes) after each step.  Returns the engine."""
    from fluidframework_amd.engine import MergeEngine
    batch, rows = localw.load(name)
    eng = MergeEngine(len(rows), ops_per_launch=b, **kw)
    if events:
        eng.enable_events(1 << 15)
    at = [0] * len(rows)
    for q, ks in enumerate(localw.steps(rows)):
        if ks != at:
            eng.apply(localw.span(batch, rows, at, ks))
        check(eng, q, rows, used_classes(eng) if ks != at else set())
        at = ks
    return eng


@pytest.mark.parametrize('b', [1, 7, 32])
@pytest.mark.parametrize('name', LOGS)
def test_engine_wide_editing_matches_reference(name, b):
    """Every checkpoint state -- pending wide inserts, pending removals, pending property changes on keys
    up to 31 -- and the end equal the reference's, at several launch sizes; no document halts.  The
    statistics show the wide editing forms, and nothing else once a document is wide; localw_offline
    reaches the forms for more than 64 pending edits; localw_promote runs in a narrow editing form up to
    its promoting launch."""
    batch, rows = localw.load(name)
    seen = set()
    first_wide = [next(i for i in range(r['n']) if localw.wide_record(batch, int(batch.row_ptr[r['doc']]) + i)) for r in rows]

    stops = localw.steps(rows)

    def check(eng, q, rows, classes):
        for i, r in enumerate(rows):
            k = stops[q][i]
            assert eng.error(i) == (0, 0), (name, r['doc'], k, eng.error(i))
            assert localw.same_state(eng, i, r, k), (name, r['doc'], k, b)
        seen.update(classes)
        # a step that every document enters wide: the wide editing forms and no other bucket
        if q > 0 and classes and all(f < k for f, k in zip(first_wide, stops[q - 1])):
            checked.append(q)
            assert all(c & CLASS_EDITING and c & CLASS_WIDE for c in classes), [hex(c) for c in classes]

    checked = []
    run_steps(name, b, check).close()
    assert len(checked) >= 2
    assert any(c & CLASS_WIDE and c & CLASS_EDITING for c in seen)
    if name == 'localw_offline':
        assert any(c & CLASS_GROUPS and c & CLASS_WIDE for c in seen), [hex(c) for c in seen]


@pytest.mark.parametrize('b', [1, 7, 32])
def test_promote_documents_run_narrow_until_they_turn_wide(b):
    """localw_promote up to (not including) each document's promoting record: a narrow editing class and
    no other; then the promoting record alone, in a wide editing class, with the reference's state on both
    sides of it."""
    from fluidframework_amd.engine import MergeEngine
    batch, rows = localw.load('localw_promote')
    ks = [r['promote']['k'] for r in rows]
    eng = MergeEngine(len(rows), ops_per_launch=b)
    eng.apply(localw.span(batch, rows, [0] * len(rows), ks))
    narrow = used_classes(eng)
    assert narrow and all(c & CLASS_EDITING and not c & CLASS_WIDE for c in narrow), [hex(c) for c in narrow]
    for i, r in enumerate(rows):
        assert eng.error(i) == (0, 0) and localw.same_state(eng, i, r, ks[i]), (r['doc'], eng.error(i))
    eng.apply(localw.span(batch, rows, ks, [k + 1 for k in ks]))
    wide = used_classes(eng)
    assert wide and all(c & CLASS_EDITING and c & CLASS_WIDE for c in wide), [hex(c) for c in wide]
    for i, r in enumerate(rows):
        assert eng.error(i) == (0, 0) and localw.same_state(eng, i, r, ks[i] + 1), (r['doc'], eng.error(i))
    eng.close()


def test_long_document_in_every_form():
    """localw_long (2100+ records, under 900 segments, few enough local edits that a launch stays in the
    forms with one group-mask word) on an engine of 8192 segments.  mt_bin_kernel picks the smallest class
    with nseg + 2 nops + n_empty + 1 <= CAP, nb[0] + 2 nops + 1 <= CAP / 2, interior blocks + nops + 1 <=
    CAP / 8 + 8 and heap + 4 nops + 16 <= CAP / 2 + 64: launches of 32 records fit a class of at most 1024
    slots (the 1024-slot wide editing form); launches of 300 need 301 interior blocks -- past the 2048
    class's 264, within the 4096 class's 520 (the 4096-slot form); launches of 1000 need 1001 -- past 520,
    within the 8192 class's 1032 (the 8192-slot form).  Two checkpoints and the end equal the reference's
    each time.  Then localw_offline's first document (past 64 pending edits) at the same launch sizes: the
    forms with MT_LOC_GW mask words at 4096 and 8192 slots."""
    from fluidframework_amd.engine import MergeEngine
    batch, rows = localw.load(LONG)
    row = rows[0]
    cks = [row['states'][1][0], row['states'][3][0], row['n']]
    assert cks[0] > 600
    for b, cap in ((32, 1024), (300, 4096), (1000, 8192)):
        eng = MergeEngine(1, seg_capacity=8192, ops_per_launch=b)
        seen, at = set(), 0
        for k in cks:
            eng.apply(localw.span(batch, rows, [at], [k]))
            seen |= used_classes(eng)
            assert eng.error(0) == (0, 0), (b, k, eng.error(0))
            assert localw.same_state(eng, 0, row, k), (b, k)
            at = k
        eng.close()
        assert CLASS_EDITING | CLASS_WIDE | cap in seen, (b, [hex(c) for c in seen])
        assert all(c & CLASS_EDITING and not c & CLASS_GROUPS for c in seen), (b, [hex(c) for c in seen])
    batch, rows = localw.load('localw_offline')
    row = rows[0]
    assert row['n'] > 600
    for b, cap in ((300, 4096), (1000, 8192)):
        eng = MergeEngine(1, seg_capacity=8192, ops_per_launch=b)
        eng.apply(localw.span(batch, [row], [0], [row['n']]))
        assert eng.error(0) == (0, 0) and localw.same_state(eng, 0, row, row['n']), (b, eng.error(0))
        assert CLASS_EDITING | CLASS_WIDE | CLASS_GROUPS | cap in used_classes(eng), (b, [hex(c) for c in used_classes(eng)])
        eng.close()


@pytest.mark.parametrize('name', LOGS + [LONG])
def test_engine_wide_editing_events_match_reference(name):
    """The editing client's callbacks (mt_events_enable), a remote annotate's over locally pending keys
    >= 8 among them: equal to the reference's (tests/golden/localw_events.jsonl)."""
    from fluidframework_amd.engine import MergeEngine
    batch, rows = localw.load(name)
    eng = MergeEngine(batch.n_docs, ops_per_launch=16).enable_events(1 << 15)
    eng.apply(batch)
    got = eng.drain_events()
    gold = localw.events(name)
    assert len(gold) == len(rows) and sum(g['n'] for g in gold) > 300
    for g in gold:
        d = g['doc']
        assert eng.error(d) == (0, 0), (name, d, eng.error(d))
        ev = got[d]
        if 'events' in g:
            assert ev == g['events'], (name, d)
        assert len(ev) == g['n'] and hashlib.sha256(json.dumps(ev, separators=(',', ':')).encode()).hexdigest() == \
            g['sha256'], (name, d)
    eng.close()


@pytest.mark.parametrize('b', [1, 16])
def test_engine_wide_reconnect_matches_reference(b):
    """Reconnect of a wide editing document: the regenerated ops (mt_regen_drain -- wide records where the
    text, a key or a value id needs them) equal the reference's, and so does every checkpoint state."""
    rows = localw.load('localw_reconnect')[1]
    stops = localw.steps(rows)
    regen = [[] for _ in rows]

    def check(eng, q, rows, classes):
        for i, r in enumerate(rows):
            k = stops[q][i]
            assert eng.error(i) == (0, 0), (r['doc'], k, eng.error(i))
            assert localw.same_state(eng, i, r, k), (r['doc'], k, b)
            # (a regenerated op names its reset record by its index in the batch applied: the step's)
            first = stops[q - 1][i] if q else 0
            regen[i] += [[first + at, ops] for at, ops in eng.regen_drain(i)]

    run_steps('localw_reconnect', b, check).close()
    for i, r in enumerate(rows):
        assert regen[i] == r['regen'], r['doc']
    assert sum(len(ops) for r in rows for _, ops in r['regen']) >= 200


@pytest.mark.parametrize('name', ['localw_lag', 'localw_promote'])
def test_local_view_reads_at_every_checkpoint(name):
    """The local view (POS_LOCAL) of a wide editing document, read from the at-rest arrays: the whole-range
    text read equals the reference's getText() (its units and their digest), and 16 positions per document resolve to the segment and
    offset of the state's own walk."""
    from fluidframework_amd.engine import POS_CONTAINING, POS_LOCAL, POS_QUERY_DTYPE, MergeEngine

    def units(seg):
        return 1 if isinstance(seg[0], dict) else len(seg[0].encode('utf-16-le', 'surrogatepass')) // 2

    def check(eng, q, rows, classes):
        docs = list(range(len(rows)))
        texts, _ = eng.text_ranges(MergeEngine.text_queries(docs))
        queries, want = [], []
        for i, r in enumerate(rows):
            k, _, _, _, text = r['states'][min(q, len(r['states']) - 1)]
            assert localw.text_digest(texts[i]) == text, (name, r['doc'], k)
            assert localw.same_state(eng, i, r, k)
            st = eng.state(i)  # (the reference's state, by its checksum: the walk below is the reference's)
            live = [(o, units(s)) for o, s in enumerate(st['segs']) if s[3] == -1 and s[4] == -1]
            total = sum(n for _, n in live)
            for p in sorted({(j * total) // 16 for j in range(16)} if total else ()):
                acc = 0
                for o, n in live:
                    if p < acc + n:
                        want.append((o, p - acc))
                        break
                    acc += n
                queries.append((i, p, POS_LOCAL, 0, POS_CONTAINING))
        res = eng.resolve_positions(np.array(queries, dtype=POS_QUERY_DTYPE))
        assert [(int(x['ordinal']), int(x['offset'])) for x in res] == want, (name, q)

    run_steps(name, 16, check).close()


def test_snapshot_of_a_wide_editing_document_with_edits_pending():
    """SnapshotV1 of localw_lag's first document cut where wide edits are pending (pending inserts and
    removals elided, snapshotV1.ts:176-241): equal to the reference's, stored with the checkpoint."""
    from fluidframework_amd.engine import MergeEngine
    batch, rows = localw.load('localw_lag')
    row = rows[0]
    k, want = row['snapshot']
    assert 'w' in next(s for s in row['states'] if s[0] == k)[3] and k < row['n']  # (a wide insert is pending there)
    names = ['observer'] + ['c%d' % i for i in range(1, 400)]
    eng = MergeEngine(1, ops_per_launch=32)
    eng.apply(localw.span(batch, [row], [0], [k]))
    assert eng.error(0) == (0, 0) and localw.same_state(eng, 0, row, k)
    assert eng.snapshot(0, 0, names) == want, k
    eng.close()


def test_refusals_that_stay():
    """On a wide editing document: an insert at a reference's leaf (MT_OP_INSERT_AT) and a local record
    with key 32 halt the document with MT_DERR_LIMITS, the 513th pending edit with MT_DERR_CAPACITY -- each
    alone: the fourth document of the launch goes on."""
    from fluidframework_amd.engine import MergeEngine
    from fluidframework_amd.oplog import ANNOTATE, INSERT, INSERT_AT, OP_DTYPE, OP_WIDE, OpBatch, build_batch
    head = [(-1, 0, 0, 1, INSERT, 0, 0, '日本語', None, 0), (-1, 0, 0, 1, INSERT, 1, 0, 'ab', {9: 300}, 0)]
    many = [(-1, 0, 0, 1, INSERT, 0, 0, '語', None, 0)] * 513
    good = build_batch([head + [(-1, 0, 0, 1, INSERT_AT, 0, 0, 'x', None, 0)],
                        head + [(-1, 0, 0, 1, ANNOTATE, 0, 2, None, {31: 7}, 0)],  # (key 31; made 32 below)
                        many,
                        head + [(-1, 0, 0, 1, ANNOTATE, 0, 2, None, {31: 65535}, 0)]])
    ops, pay = good.ops.copy(), good.payload.copy()
    bad = ops[int(good.row_ptr[1]) + 2]
    assert bad['type'] & OP_WIDE and pay[bad['payload_off']] == 31
    pay[bad['payload_off']] = 32
    batch = OpBatch(ops.astype(OP_DTYPE), pay, good.row_ptr)
    for b in (1, 32):
        eng = MergeEngine(4, ops_per_launch=b)
        eng.apply(batch)
        assert eng.error(0)[0] == MT_DERR_LIMITS and eng.error(1)[0] == MT_DERR_LIMITS, (eng.error(0), eng.error(1))
        assert eng.error(2)[0] == MT_DERR_CAPACITY, eng.error(2)
        assert eng.error(3) == (0, 0)
        assert len(eng.state(2)['segs']) == 512 and all(s[1] == -1 for s in eng.state(2)['segs'])
        st = eng.state(3)
        assert [s[0] for s in st['segs']] == ['日', 'a', 'b', '本語']
        assert [s[6] for s in st['segs']] == [{'k31': 65535}, {'k9': 300, 'k31': 65535}, {'k9': 300}, None]
        eng.close()
