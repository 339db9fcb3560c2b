"""Interval collections (include/mtgpu.h "interval collections") against the reference's own
intervalCollection.ts.

tests/golden/intervals.expected.jsonl (make_intervals.py, intervals_ref.js) holds, for the first
documents of seven logs, the queries, deletes and adds a seeded plan executed on the reference at
message boundaries: for every query the intervals x with x.overlaps(query) -- the per-interval answer
the engine gives -- beside what the reference's stale tree answered, and at every step each live
interval's ends as (ordinal, raw offset, toPosition()).  The engine follows the same steps -- the batch
cut at the plan's record counts -- and must give the same handles, delete results, overlap sets and
positions.  An interval with an end on a segment zamboni unlinked is left out of a query's comparison
(the reference compares a stale ordinal string there; include/mtgpu.h): at most 1 % of the pairs.
"""
import hashlib
import json
import os
import shutil
import sys

import numpy as np
import pytest

from conftest import GOLDEN

LOGS = ('intervals_spec', 'scenarios', 'markers', 'wide', 'synth_c3', 'local_lag', 'local_offline')
EVCAP = 1 << 17
PER_DOC = 256


def load_fixture():
    with open(os.path.join(GOLDEN, 'intervals.expected.jsonl')) as f:
        lines = [json.loads(x) for x in f if x.strip()]
    by_log = {}
    for r in lines[1:]:
        by_log.setdefault(r['log'], []).append(r)
    return lines[0], by_log


def load_log(name):
    from fluidframework_amd.oplog import OpBatch
    return OpBatch.load(os.path.join(GOLDEN, name + '.mtlog'))


def cut(batch, docs, lo, hi):
    """records [lo[i], hi[i]) of document docs[i], as one batch over the documents in that order"""
    from fluidframework_amd.oplog import OpBatch
    idx, rp = [], [0]
    for d, a, b in zip(docs, lo, hi):
        base = int(batch.row_ptr[d])
        idx.append(np.arange(base + a, base + b))
        rp.append(rp[-1] + b - a)
    idx = np.concatenate(idx) if idx else np.zeros(0, np.int64)
    return OpBatch(batch.ops[idx.astype(np.int64)].copy(), batch.payload, np.array(rp, dtype=np.uint32))


def digest(x):
    return hashlib.sha256(json.dumps(x, separators=(',', ':')).encode()).hexdigest()


def end(o, off):
    return (None if o < 0 else o, off)


def test_fixture_shape():
    head, by_log = load_fixture()
    c = head['counts']
    assert set(by_log) == set(LOGS)
    assert c['slid'] > 0 and c['detached_remove'] > 0 and c['born_detached'] > 0 and c['max_live'] > 64
    assert 0 < c['tree_exact'] <= c['queries'] and c['deletes'] > 0 and c['adds'] > 0
    assert c['unlinked_pairs'] * 100 <= c['pairs']  # the condition on what the comparisons leave out
    queries = pairs = unlinked = 0
    for name, rows in by_log.items():
        batch = load_log(name)
        assert [r['doc'] for r in rows] == list(range(len(rows)))
        for r in rows:
            assert r['err'] is None
            n = int(batch.row_ptr[r['doc'] + 1] - batch.row_ptr[r['doc']])
            ks = [s['k'] for s in r['steps']]
            assert ks == sorted(set(ks)) and ks[-1] == n, (name, r['doc'], ks, n)
            live, nxt = set(), 0
            for s in r['steps']:
                full = not isinstance(s['check'], str)
                assert full == (r['doc'] < 2)
                if full:
                    assert [x[0] for x in s['check']] == sorted(live), (name, r['doc'], s['k'])
                    # toPosition() is -1 exactly without a linked segment
                    assert all((x[1] < 0) == (x[3] < 0) and (x[4] < 0) == (x[6] < 0) for x in s['check'])
                for op in s['ops']:
                    if op[0] == 'q':
                        queries += 1
                        pairs += len(live)
                        if full:
                            assert set(op[4]) <= set(op[3]) <= live  # the tree's answer: a subset
                            unlinked += len(op[7]) if len(op) > 7 else 0
                        else:
                            unlinked += len(op[3]) if len(op) > 3 else 0
                    elif op[0] == 'd':
                        assert op[1] in live and op[2] >= 0 and op[3] >= 0
                        live.discard(op[1])
                    else:
                        assert op[0] == 'a' and op[1] == nxt and 0 <= op[2] <= op[3] and op[4] in (0, 1, 2)
                        nxt += 1
                        live.add(op[1])
    assert (queries, pairs, unlinked) == (c['queries'], c['pairs'], c['unlinked_pairs'])


def test_python_overlaps_reproduces_the_reference():
    """intervals.overlaps, fed each query's recorded ends and the step's recorded interval ends,
    gives every fully recorded per-interval answer (intervals with an end on an unlinked segment left
    out)."""
    from fluidframework_amd.intervals import overlaps
    head, by_log = load_fixture()
    pairs = left_out = queries = 0
    for name, rows in by_log.items():
        for r in rows:
            for s in r['steps']:
                if isinstance(s['check'], str):
                    continue
                for op in s['ops']:
                    if op[0] != 'q':
                        break  # (a step's queries come first: the check is their state)
                    out = set(op[7]) if len(op) > 7 else set()
                    q = (end(*op[5]), end(*op[6]))
                    got = [x[0] for x in s['check']
                           if x[0] not in out and overlaps((end(x[1], x[2]), end(x[4], x[5])), q)]
                    assert got == [i for i in op[3] if i not in out], (name, r['doc'], s['k'], op)
                    pairs += len(s['check'])
                    left_out += len(out)
                    queries += 1
    # (the 1 % condition is on the whole fixture: test_fixture_shape recounts it against the header)
    assert queries > 300 and left_out <= head['counts']['unlinked_pairs'], (queries, left_out, pairs)


def test_python_compare_rules():
    from fluidframework_amd.intervals import compare, equal, overlaps, ref_types
    assert compare((3, 5), (3, 2)) > 0 and compare((None, 1), (None, 4)) < 0 and compare((None, 0), (None, 0)) == 0
    assert compare((None, 9), (0, 0)) == -1 and compare((0, 0), (None, 9)) == 1 and compare((2, 9), (3, 0)) == -1
    # both of the query's ends undefined (past the end): the offset difference decides
    assert overlaps(((None, 0), (None, 0)), ((None, 0), (None, 0))) is False
    assert overlaps(((1, 0), (None, 0)), ((None, 0), (None, 0))) is False
    assert overlaps(((None, 0), (4, 1)), ((2, 0), (2, 3))) and not overlaps(((3, 0), (4, 1)), ((2, 0), (2, 3)))
    assert equal(((1, 2), (None, 0)), ((1, 2), (None, 0))) and not equal(((1, 2), (3, 0)), ((1, 2), (3, 1)))
    assert ref_types(0) == (0x10, 0x20) and ref_types(1) == (0x2, 0x4) and ref_types(2) == (0x50, 0x60)
    assert ref_types(3) == (0x50, 0x60)  # Nest | SlideOnRemove is not Nest (intervalCollection.ts:215)


HAVE_REF = os.path.isdir('/root/reference/packages/dds/sequence/src') and shutil.which('node')


@pytest.mark.reference
@pytest.mark.skipif(not HAVE_REF, reason='reference sources / node not present (GPU box)')
def test_fixture_regenerates_byte_identically():
    sys.path.insert(0, GOLDEN)
    import make_intervals
    text, spec, _ = make_intervals.generate()
    with open(os.path.join(GOLDEN, 'intervals.expected.jsonl')) as f:
        assert f.read() == text
    kept = load_log('intervals_spec')
    assert np.array_equal(kept.ops, spec.ops) and np.array_equal(kept.payload, spec.payload) and \
        np.array_equal(kept.row_ptr, spec.row_ptr)


def _engine(n, b, per_doc=PER_DOC, refs=None, evcap=EVCAP, **kw):
    from fluidframework_amd.engine import MergeEngine
    eng = MergeEngine(n, ops_per_launch=b, **kw).enable_events(evcap).enable_refs(refs or 2 * per_doc)
    return eng.enable_intervals(per_doc)


def follow(eng, batch, rows):
    """The fixture's executed steps of `rows` (one per engine document) on the engine.  Asserts the add
    handles (the lowest free entry), the delete results, the overlap sets and the positions of fully
    recorded steps; returns per document, per step, the digest of the answers (hashed steps)."""
    from fluidframework_amd.refs import REF_NONE
    docs = [r['doc'] for r in rows]
    n_steps = max(len(r['steps']) for r in rows)
    at = [0] * len(rows)
    handle = [dict() for _ in rows]  # id -> handle, live intervals in id order
    digests = [[] for _ in rows]
    pairs = left_out = 0
    for s in range(n_steps):
        on = [i for i, r in enumerate(rows) if s < len(r['steps'])]
        hi = [r['steps'][s]['k'] if s < len(r['steps']) else at[i] for i, r in enumerate(rows)]
        eng.apply(cut(batch, docs, at, hi))
        at = hi
        where = lambda i: (rows[i]['log'], rows[i]['doc'], rows[i]['steps'][s]['k'])
        # the check: every live interval's toPosition() pair, and no other entry is live
        pos = eng.interval_positions(on)
        answers = {}
        for j, i in enumerate(on):
            assert sorted(np.nonzero(pos[j]['live'])[0].tolist()) == sorted(handle[i].values()), where(i)
            got = [[rid, int(pos[j][h]['start']), int(pos[j][h]['end'])] for rid, h in handle[i].items()]
            answers[i] = [got]
            chk = rows[i]['steps'][s]['check']
            if not isinstance(chk, str):
                assert got == [[x[0], x[3], x[6]] for x in chk], where(i)
        # the queries come first, all documents' in one call
        qs = [(i, op) for i in on for op in rows[i]['steps'][s]['ops'] if op[0] == 'q']
        hs, rp = eng.overlapping_intervals([i for i, _ in qs], [op[1] for _, op in qs], [op[2] for _, op in qs])
        for j, (i, op) in enumerate(qs):
            by_handle = {h: rid for rid, h in handle[i].items()}
            row = hs[rp[j]:rp[j + 1]].tolist()
            assert row == sorted(row), where(i)
            full = len(op) > 4
            out = set(op[7] if full and len(op) > 7 else op[3] if not full and len(op) > 3 else [])
            got = sorted(by_handle[h] for h in row if by_handle[h] not in out)
            answers[i].append(got)
            pairs += len(handle[i])
            left_out += len(out)
            if full:
                assert got == [x for x in op[3] if x not in out], (where(i), op)
                assert set(op[4]) - out <= set(got), (where(i), op)  # the tree's answer: a subset
        for i in on:
            digests[i].append(digest(answers[i]))
        # deletes and adds, one op of each document per call: handles are handed out in a known order
        rest = {i: [op for op in rows[i]['steps'][s]['ops'] if op[0] != 'q'] for i in on}
        for j in range(max([len(v) for v in rest.values()] or [0])):
            dels = [(i, v[j]) for i, v in rest.items() if j < len(v) and v[j][0] == 'd']
            adds = [(i, v[j]) for i, v in rest.items() if j < len(v) and v[j][0] == 'a']
            if dels:
                gone = eng.remove_intervals([i for i, _ in dels], [op[2] for _, op in dels], [op[3] for _, op in dels])
                for (i, op), h in zip(dels, gone.tolist()):
                    assert h != REF_NONE and h == handle[i].pop(op[1]), (where(i), op, h)
            if adds:
                new = eng.add_intervals([i for i, _ in adds], [op[2] for _, op in adds], [op[3] for _, op in adds],
                                        [op[4] for _, op in adds])
                for (i, op), h in zip(adds, new.tolist()):
                    used = set(handle[i].values())
                    assert h == min(x for x in range(len(used) + 1) if x not in used), (where(i), op, h)
                    handle[i][op[1]] = h
    return digests, pairs, left_out


@pytest.mark.gpu
@pytest.mark.parametrize('b', [1, 7, 32])
@pytest.mark.parametrize('name', LOGS)
def test_engine_intervals_match_reference(name, b):
    """Add handles, delete results, overlap sets (the per-interval answer; the tree's a subset) and
    interval positions of every step, exactly; no document errs."""
    rows = load_fixture()[1][name]
    batch = load_log(name)
    eng = _engine(len(rows), b)
    digests, pairs, left_out = follow(eng, batch, rows)
    for i, r in enumerate(rows):
        assert eng.error(i) == (0, 0), (name, r['doc'], eng.error(i))
        for s, st in enumerate(r['steps']):
            if isinstance(st['check'], str):
                assert st['check'] == digests[i][s], (name, r['doc'], b, st['k'])
    eng.close()


def _restate(eng, doc, ivs, s, e):
    """findOverlappingIntervals(s, e) on document `doc` from ref_positions-style facts: `ivs` is
    {handle: ((ordinal | None, raw offset), (ordinal | None, raw offset))}."""
    from fluidframework_amd.engine import POS_CONTAINING, POS_LOCAL, POS_QUERY_DTYPE
    from fluidframework_amd.intervals import overlaps
    q = np.zeros(2, dtype=POS_QUERY_DTYPE)
    q['doc'], q['pos'], q['ref_seq'], q['kind'] = doc, [s, e], POS_LOCAL, POS_CONTAINING
    at = eng.resolve_positions(q)
    tr = tuple((int(a['ordinal']), int(a['offset'])) if a['ordinal'] >= 0 and p >= 0 else (None, 0)
               for a, p in zip(at, (s, e)))
    return sorted(h for h, iv in ivs.items() if overlaps(iv, tr))


@pytest.mark.gpu
def test_wave_boundary_shapes():
    """A document of more than 130 leaves (alternating clients' one-character inserts) with 70 and then
    129 intervals (two and three lane chunks): queries with ends in leaf 0, leaves 63 / 64, the last
    leaf, at the length and one past it, against a host restatement (intervals.overlaps over each
    interval's ends from where getContainingSegment put them); an interval with both ends on one
    tombstone; an end detached from birth against a query past the end (both undefined: the offset
    difference); a batch where most documents hold no intervals; zero queries."""
    from fluidframework_amd.engine import POS_CONTAINING, POS_LOCAL, POS_QUERY_DTYPE
    from fluidframework_amd.oplog import INSERT, OP_DTYPE, REMOVE, OpBatch
    n_leaves, n_docs, D = 140, 6, 2
    rows = [(i + 1, i, 0, 1 + i % 2, INSERT, 0, i, 0, i, 1) for i in range(n_leaves)]  # msn 0: nothing is appended
    payload = np.frombuffer(bytes(97 + i % 26 for i in range(n_leaves)), dtype=np.uint8)
    rp = [0] * (D + 1) + [n_leaves] * (n_docs - D)
    eng = _engine(n_docs, 32, per_doc=160)
    eng.apply(OpBatch(np.array(rows, dtype=OP_DTYPE), payload, np.array(rp, dtype=np.uint32)))
    assert eng.seg_counts()[D] == n_leaves and eng.length(D) == n_leaves and eng.length(0) == 0

    def containing(ps):
        q = np.zeros(len(ps), dtype=POS_QUERY_DTYPE)
        q['doc'], q['pos'], q['ref_seq'], q['kind'] = D, ps, POS_LOCAL, POS_CONTAINING
        return [(int(a['ordinal']), int(a['offset'])) if a['ordinal'] >= 0 else (None, 0) for a in eng.resolve_positions(q)]

    ivs = {}

    def add(starts, ends, types):
        hs = eng.add_intervals([D] * len(starts), starts, ends, types).tolist()
        for h, a, b in zip(hs, containing(starts), containing(ends)):
            assert h < 160 and h not in ivs
            ivs[h] = (a, b)
        return hs

    queries = [(0, 0), (0, 1), (0, 63), (63, 64), (64, 64), (62, 65), (0, n_leaves - 1), (n_leaves - 1, n_leaves - 1),
               (n_leaves - 1, n_leaves), (0, n_leaves), (0, n_leaves + 1), (n_leaves, n_leaves + 1), (64, n_leaves + 1),
               (127, 128), (128, 139), (30, 30)]

    def check():
        # the restatement's facts are what ref_positions says of every interval's two references
        # (getOffset() is the raw offset here: no end sits past offset 0 of a removed leaf)
        pos = eng.interval_positions([D])[0]
        live = [h for h in range(len(pos)) if pos[h]['live'] and pos[h]['collection'] == 0]
        assert live == sorted(ivs)
        at = eng.ref_positions([D] * (2 * len(live)), [int(pos[h][k]) for h in live for k in ('start_ref', 'end_ref')])
        ends = [(None if a['ordinal'] < 0 else int(a['ordinal']), int(a['offset'])) for a in at]
        assert {h: (ends[2 * j], ends[2 * j + 1]) for j, h in enumerate(live)} == ivs
        hs, rp = eng.overlapping_intervals([D] * len(queries), [q[0] for q in queries], [q[1] for q in queries])
        for j, (s, e) in enumerate(queries):
            assert hs[rp[j]:rp[j + 1]].tolist() == _restate(eng, D, ivs, s, e), (s, e, len(ivs))
        return hs, rp

    first = add([2 * j for j in range(70)], [min(2 * j + j % 5, n_leaves + 1) for j in range(70)], [j % 3 for j in range(70)])
    assert sorted(first) == list(range(70))
    hs, rp = check()
    # (0, last character): every interval with an attached end, past one lane chunk; (0, length) has an
    # undefined end, below which no attached start sorts: nothing
    assert rp[7] - rp[6] == 69 and rp[10] - rp[9] == 0
    # (every other one ends at or past the length: an end without a segment)
    add([j + 1 for j in range(58)], [n_leaves + (j // 2) % 2 if j % 2 else j + 4 for j in range(58)], [2] * 58)
    born = add([n_leaves + 3], [n_leaves + 5], [0])  # both ends detached from birth
    assert len(ivs) == 129 and max(ivs) == 128 and ivs[born[0]] == ((None, 0), (None, 0))
    hs, rp = check()
    # a query past the end has both ends undefined, as the born-detached interval's: 0 - 0 < 0 is false
    past = eng.overlapping_intervals([D], [n_leaves + 1], [n_leaves + 9])
    assert past[0].tolist() == _restate(eng, D, ivs, n_leaves + 1, n_leaves + 9) and born[0] not in past[0].tolist()
    # another collection of the same document: its interval is seen by its own queries and removes only
    other = eng.add_intervals([D], [5], [9], [0], collections=3).tolist()
    assert other == [129]
    check()
    assert eng.overlapping_intervals([D], [0], [n_leaves - 1], collections=3)[0].tolist() == other
    assert eng.remove_intervals([D], [5], [9]).tolist() == [0xFFFFFFFF]
    assert eng.remove_intervals([D], [5], [9], collections=3).tolist() == other
    assert len(eng.overlapping_intervals([D], [0], [n_leaves - 1], collections=3)[0]) == 0
    # most documents hold no intervals; document ids past the batch's documents answer empty too
    mixed_d = [0, 1, D, 3, 4, 5, D, 0]
    hs, rp = eng.overlapping_intervals(mixed_d, [0] * 8, [n_leaves - 1] * 8)
    want = _restate(eng, D, ivs, 0, n_leaves - 1)
    assert len(want) > 64 and [int(rp[j + 1] - rp[j]) for j in range(8)] == [0, 0, len(want), 0, 0, 0, len(want), 0]
    assert hs.tolist() == want + want
    # zero queries
    hs, rp = eng.overlapping_intervals([], [], [])
    assert len(hs) == 0 and rp.tolist() == [0]
    # both ends on one tombstone: client 2 removes leaves 104..105, then client 1, which has not seen
    # that, removes leaves 100..103: its SlideOnRemove ends slide to leaf 104, a tombstone here (the
    # observer keeps removed leaves linked until the msn passes); other ends are detached and keep
    # their raw offset (0 on these one-character leaves)
    tomb = add([101], [101], [0])
    two = np.array([(n_leaves + 1, n_leaves, 0, 2, REMOVE, 0, 104, 106, 0, 0),
                    (n_leaves + 2, n_leaves, 0, 1, REMOVE, 0, 100, 104, 0, 0)], dtype=OP_DTYPE)
    eng.apply(OpBatch(two, payload, np.array([0] * D + [0, 2] + [2] * (n_docs - D - 1), dtype=np.uint32)))
    assert eng.error(D) == (0, 0) and eng.length(D) == n_leaves - 6 and eng.seg_counts()[D] == n_leaves
    pos = eng.interval_positions([D])[0]
    types = {h: int(pos[h]['interval_type']) for h in ivs}

    def moved(e, t, lo, hi):
        if e[0] is None or not lo <= e[0] < hi:
            return e
        return (hi, 0) if t & 2 else (None, e[1])
    for lo, hi in ((104, 106), (100, 104)):
        for h in list(ivs):
            ivs[h] = (moved(ivs[h][0], types[h], lo, hi), moved(ivs[h][1], types[h], lo, hi))
    assert ivs[tomb[0]] == ((None, 0), (None, 0)) and ivs[first[50]] == ((104, 0), (104, 0))
    assert (int(pos[tomb[0]]['start']), int(pos[tomb[0]]['end'])) == (-1, -1) and pos[tomb[0]]['live'] == 1
    assert (int(pos[first[50]]['start']), int(pos[first[50]]['end'])) == (100, 100)
    ln = n_leaves - 6
    queries[:] = [(0, 0), (99, 100), (100, 101), (100, 100), (0, ln - 1), (0, ln), (0, ln + 1), (96, 99), (63, 64),
                  (110, 120), (ln + 1, ln + 2)]
    check()
    eng.close()


@pytest.mark.gpu
def test_lifecycle():
    """enable_intervals needs enable_refs with room for two references each; a full interval table, or a
    full reference table, refuses the add with REF_FULL and leaves no stray reference (the reference
    slots in use are unchanged); a removed interval's entry is reusable while its two references stay;
    disabling, reset and a snapshot load free the intervals."""
    from fluidframework_amd import snapshot
    from fluidframework_amd.engine import MergeEngine, MtError
    from fluidframework_amd.refs import REF_FULL, REF_NONE
    batch = load_log('synth_c3')
    n = 3
    eng = MergeEngine(n, ops_per_launch=32).enable_events(EVCAP)
    with pytest.raises(MtError, match='bad argument'):
        eng.enable_intervals(4)  # before enable_refs
    eng.enable_refs(8)
    with pytest.raises(MtError, match='bad argument'):
        eng.enable_intervals(5)  # 10 references do not fit
    eng.enable_intervals(2)
    eng.apply(cut(batch, range(n), [0] * n, [200] * n))
    ln = eng.length(1)
    assert ln > 12

    def ref_slots_free(d):  # how many more references document d's table takes
        hs = []
        while True:
            h = int(eng.add_refs([d], [0], [0])[0])
            if h == REF_FULL:
                break
            hs.append(h)
        eng.remove_refs([d] * len(hs), hs)
        return len(hs)

    assert ref_slots_free(1) == 8
    assert eng.add_intervals([1], [1], [2], [0]).tolist() == [0]
    assert eng.add_intervals([1], [3], [4], [2]).tolist() == [1]
    assert ref_slots_free(1) == 4
    # the interval table is full: refused, and no reference slot was taken
    assert eng.add_intervals([1], [5], [6], [0]).tolist() == [REF_FULL]
    assert ref_slots_free(1) == 4
    assert eng.overlapping_intervals([1], [0], [ln - 1])[0].tolist() == [0, 1]
    # a removed interval frees its entry; its two references stay (removeInterval never calls
    # removeLocalReference)
    assert eng.remove_intervals([1, 1], [1, 1], [3, 2]).tolist() == [REF_NONE, 0]
    assert ref_slots_free(1) == 4
    assert eng.add_intervals([1], [5], [6], [0]).tolist() == [0]
    assert ref_slots_free(1) == 2
    # the reference table is full part-way through an add: the start's slot is handed back
    assert eng.remove_intervals([1], [5], [6]).tolist() == [0]
    own = eng.add_refs([1], [0], [0])
    assert ref_slots_free(1) == 1
    assert eng.add_intervals([1], [7], [8], [2]).tolist() == [REF_FULL]
    assert ref_slots_free(1) == 1 and int(eng.interval_positions([1])[0]['live'].sum()) == 1
    eng.remove_refs([1], own)
    assert eng.add_intervals([1], [7], [8], [2]).tolist() == [0]
    # the document keeps running, other documents are untouched
    eng.apply(cut(batch, range(n), [200] * n, [400] * n))
    assert all(eng.error(d) == (0, 0) for d in range(n))
    assert eng.overlapping_intervals([0, 2], [0, 0], [eng.length(0), eng.length(2)])[1].tolist() == [0, 0, 0]
    # a snapshot load of a document frees that document's intervals, and no other's
    assert eng.add_intervals([0], [0], [1], [0]).tolist() == [0]
    snapshot.load_docs(eng, [eng.snapshot(1)], doc_ids=[1])
    assert int(eng.interval_positions([1])[0]['live'].sum()) == 0 and ref_slots_free(1) == 8
    assert int(eng.interval_positions([0])[0]['live'].sum()) == 1
    # reset (mt_docs_init) frees the intervals with the references
    eng.reset()
    assert int(eng.interval_positions([0])[0]['live'].sum()) == 0
    # disabling frees the tables: the calls are refused; enabling again starts empty
    eng.enable_intervals(0)
    with pytest.raises(MtError, match='bad argument'):
        eng.overlapping_intervals([0], [0], [1])
    eng.enable_intervals(2)
    assert eng.overlapping_intervals([0], [0], [1])[1].tolist() == [0, 0]
    eng.enable_refs(0)  # frees the intervals with the references
    with pytest.raises(MtError, match='bad argument'):
        eng.add_intervals([0], [0], [1], [0])
    eng.close()
