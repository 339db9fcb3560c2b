"""Checkpoints of editing clients' documents on the device (include/mtgpu.h "document checkpoints",
DESIGN.md "Checkpoints"): engine A applies a prefix of a log that ends where edits are pending, saves
its documents and is closed; engine B, another object with seg_capacity 4096, restores them into its
slots in reversed order, saves the same bytes at once, and applies the rest.

Every expectation is the reference's fixture (the states, callbacks and regenerated ops of reference
clients replaying the logs), never an uninterrupted run of the engine.  The states B reaches witness the
restored pending groups, property counts and stamps; the callbacks the heap order, needsScour and the
groups' ack order; the regenerated ops the records a reconnect had produced and not handed over yet.
"""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import localw
from conftest import GOLDEN, load_golden
from test_checkpoint_gpu import _part
from test_local import LOGS, RECONNECT, load_local

pytestmark = pytest.mark.gpu

MT_SEQ_REGEN = -2
HUGE, OFFLINE, OFFLINE_LONG = 'local_huge', 'local_offline', 'local_offline_long'


def _engine(n, b=0, **kw):
    from fluidframework_amd.engine import MergeEngine
    return MergeEngine(n, ops_per_launch=b, **kw)


@functools.lru_cache(maxsize=None)
def _log(name):
    """(batch, rows) of a narrow editing log: rows are the fixture's records of its documents."""
    from fluidframework_amd.oplog import OpBatch
    batch = OpBatch.load(os.path.join(GOLDEN, name + '.mtlog'))
    if name in LOGS or name == RECONNECT:
        return batch, load_local()[name]
    with open(os.path.join(GOLDEN, name + '.expected.jsonl')) as f:
        return batch, [json.loads(x) for x in f]


def _span(batch, rows, lo, hi):
    """records [lo[i], hi[i]) of every row's document, in the rows' order (test_checkpoint_gpu._part)"""
    a, b = np.zeros(batch.n_docs, np.int64), np.zeros(batch.n_docs, np.int64)
    for r, x, y in zip(rows, lo, hi):
        a[r['doc']], b[r['doc']] = x, y
    return _part(batch, a, b, order=[r['doc'] for r in rows])


def _place(batch, n_slots, items):
    """A batch of n_slots documents: slot s carries records [lo, hi) of the log's document doc for every
    (s, doc, lo, hi) of items, and nothing for the other slots (_part carries one document per slot)."""
    from fluidframework_amd.oplog import OpBatch
    by_slot = {s: (d, a, b) for s, d, a, b in items}
    idx, rp = [], [0]
    for s in range(n_slots):
        if s in by_slot:
            d, a, b = by_slot[s]
            base = int(batch.row_ptr[d])
            idx.append(np.arange(base + a, base + b))
            rp.append(rp[-1] + b - a)
        else:
            rp.append(rp[-1])
    ix = np.concatenate(idx).astype(np.int64) if idx else np.zeros(0, np.int64)
    return OpBatch(batch.ops[ix].copy(), batch.payload, np.array(rp, dtype=np.uint32))


def _narrow_same(eng, i, row, k):
    """the engine's document i is in the reference's state after row's first k records (where the fixture
    has a checkpoint there)"""
    for kk, want in row['states']:
        if kk == k:
            assert eng.state(i) == want, (row['log'], row['doc'], k)
    return True


def _wide_same(eng, i, row, k):
    if any(s[0] == k for s in row['states']):
        assert localw.same_state(eng, i, row, k)
    return True


def _restored(blob, n, b, events=0):
    """engine B: document d of the blob in slot n - 1 - d; its own blob right after is the same bytes"""
    bb = _engine(n, b, seg_capacity=4096)
    if events:
        bb.enable_events(events)
    rev = np.arange(n, dtype=np.uint32)[::-1].copy()
    bb.restore_docs(blob, docs=rev)
    assert np.array_equal(bb.save_docs(docs=rev), blob)
    return bb


def _save_at(batch, rows, cut, b, same, **kw):
    """engine A: every row's first cut[i] records; (blob, its description)"""
    from fluidframework_amd import checkpoint
    n = len(rows)
    a = _engine(n, b, **kw)
    a.apply(_span(batch, rows, [0] * n, cut))
    for i, r in enumerate(rows):
        assert a.error(i) == (0, 0), (r['log'], r['doc'], cut[i], a.error(i))
        same(a, i, r, cut[i])
    blob = a.save_docs()
    a.close()
    desc = checkpoint.describe(blob)
    assert len(desc) == n and all('editing' in x['classes'] for x in desc)
    return blob, desc


def _continue(bb, batch, rows, cut, later, same):
    """B (slots reversed) from cut through the stops of `later` (one list of record counts per step)"""
    rr, at = rows[::-1], list(cut[::-1])
    for ks in later:
        ks = [max(k, c) for k, c in zip(ks[::-1], at)]
        if ks != at:
            bb.apply(_span(batch, rr, at, ks))
        for s, r in enumerate(rr):
            assert bb.error(s) == (0, 0), (r['log'], r['doc'], ks[s], bb.error(s))
            same(bb, s, r, ks[s])
        at = ks
    assert at == [r['states'][-1][0] for r in rr]


def _through(batch, rows, cut, later, b, same, **kw):
    blob, desc = _save_at(batch, rows, cut, b, same, **kw)
    bb = _restored(blob, len(rows), b)
    _continue(bb, batch, rows, cut, later, same)
    bb.close()
    return desc


def _fixture_pending(state):
    return any(s[1] == -1 or (s[3] == -1 and s[4] != -1) for s in state['segs'])


# ---- 1. narrow editing documents, cut at every checkpoint ------------------------------------------
@pytest.mark.parametrize('b', [7, 32])
@pytest.mark.parametrize('name', LOGS)
def test_narrow_editing_documents_cut_at_every_checkpoint(name, b):
    """A's states at the cut, and B's at every later checkpoint and at the end, are the reference's; nothing
    halts.  Over all cuts at least as many saved documents carry pending groups as fixture states at the
    cuts show a pending segment (28 / 69 / 8 / 25 of the logs' pairs), at least 8."""
    batch, rows = _log(name)
    stops = localw.steps(rows)
    blob_pending = fixture_pending = 0
    for q in range(len(stops) - 1):
        desc = _through(batch, rows, stops[q], stops[q + 1:], b, _narrow_same)
        blob_pending += sum(1 for x in desc if x['pending'] > 0)
        fixture_pending += sum(1 for r in rows if _fixture_pending(r['states'][q][1]))
    assert blob_pending >= fixture_pending >= 8, (name, blob_pending, fixture_pending)


# ---- 2. callbacks across the restore ---------------------------------------------------------------
def _gold_events(name, path='local_events.jsonl'):
    with open(os.path.join(GOLDEN, path)) as f:
        return [g for g in map(json.loads, f) if g.get('log', name) == name]


def _events_match(g, ev):
    if 'events' in g:
        assert ev == g['events'], (g.get('log'), g['doc'])
    assert len(ev) == g['n'] and \
        hashlib.sha256(json.dumps(ev, separators=(',', ':')).encode()).hexdigest() == g['sha256'], (g.get('log'), g['doc'])


@pytest.mark.parametrize('name', LOGS + [RECONNECT])
def test_callbacks_across_the_restore(name):
    """Events on in both engines, cut at each document's middle checkpoint, A drained before it saves: A's
    callbacks followed by B's are the reference's (tests/golden/local_events.jsonl)."""
    batch, rows = _log(name)
    n = len(rows)
    cut = [r['states'][(len(r['states']) - 1) // 2][0] for r in rows]  # (never the last: B has records left)
    end = [r['states'][-1][0] for r in rows]
    assert all(c < e for c, e in zip(cut, end))
    a = _engine(n, 16).enable_events(1 << 15)
    a.apply(_span(batch, rows, [0] * n, cut))
    ev_a = a.drain_events()
    blob = a.save_docs()
    a.close()
    bb = _restored(blob, n, 16, events=1 << 15)
    bb.apply(_span(batch, rows[::-1], cut[::-1], end[::-1]))
    ev_b = bb.drain_events()
    gold = {g['doc']: g for g in _gold_events(name)}
    assert sum(len(e) for e in ev_a) > 100 and sum(len(e) for e in ev_b) > 100
    for i, r in enumerate(rows):
        assert bb.error(n - 1 - i) == (0, 0), (name, r['doc'], bb.error(n - 1 - i))
        _events_match(gold[r['doc']], ev_a[i] + ev_b[n - 1 - i])
    bb.close()


# ---- 3. a reconnect cut in the middle ----------------------------------------------------------------
def _regen_cut(batch, row, run=2):
    """right after the first record of the document's first run of at least `run` MT_SEQ_REGEN records"""
    a = int(batch.row_ptr[row['doc']])
    seq = batch.ops['seq'][a:a + row['states'][-1][0]]
    for i in range(len(seq) - run + 1):
        if all(seq[i + j] == MT_SEQ_REGEN for j in range(run)):
            return i + 1
    raise AssertionError((row['doc'], 'no run of regenerating records'))


def _through_reconnect(batch, rows, b, same):
    from fluidframework_amd import checkpoint
    n = len(rows)
    cut = [_regen_cut(batch, r) for r in rows]
    end = [r['states'][-1][0] for r in rows]
    a = _engine(n, b)
    a.apply(_span(batch, rows, [0] * n, cut))  # (not drained: the regenerated ops travel in the blob)
    blob = a.save_docs()
    a.close()
    assert all(x['pending'] > 0 and 'editing' in x['classes'] for x in checkpoint.describe(blob))
    bb = _restored(blob, n, b)
    for i, r in enumerate(rows):
        before = [e for e in r['regen'] if e[0] < cut[i]]
        assert before and bb.regen_drain(n - 1 - i) == before, r['doc']
    bb.apply(_span(batch, rows[::-1], cut[::-1], end[::-1]))
    for i, r in enumerate(rows):
        s = n - 1 - i
        assert bb.error(s) == (0, 0), (r['doc'], bb.error(s))
        # (a header's record index counts within the batch that carried the record: B's restart at the cut)
        got = [[at + cut[i], ops] for at, ops in bb.regen_drain(s)]
        assert got and got == [e for e in r['regen'] if e[0] >= cut[i]], r['doc']
        same(bb, s, r, end[i])
    bb.close()


def test_reconnect_cut_in_the_middle_regenerated_ops_not_drained():
    batch, rows = _log(RECONNECT)
    assert len(rows) == 24
    _through_reconnect(batch, rows, 16, _narrow_same)


# ---- 4. the group-pool row -----------------------------------------------------------------------------
@pytest.mark.parametrize('name,q', [(OFFLINE, 1), (OFFLINE, 3), (OFFLINE_LONG, 1)])
def test_group_pool_row(name, q):
    """More than 64 edits pending at the cut (MT_WIDE_GROUPS: gmx and mt_locx travel); B goes on to the
    reference's states at every later checkpoint."""
    batch, rows = _log(name)
    stops = localw.steps(rows)
    desc = _through(batch, rows, stops[q], stops[q + 1:], 32, _narrow_same)
    assert any('groups' in x['classes'] and x['pending'] > 64 for x in desc), desc


# ---- 5. the big-pool row -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _huge_blob():
    """local_huge cut at its checkpoint 4 (1,348 and 1,252 segments, edits pending): A's blob, made once"""
    batch, rows = _log(HUGE)
    return _save_at(batch, rows, localw.steps(rows)[4], 32, _narrow_same)


def test_big_pool_row():
    batch, rows = _log(HUGE)
    stops = localw.steps(rows)
    blob, desc = _huge_blob()
    assert all(x['nseg'] > 1024 and 'editing' in x['classes'] and x['pending'] > 0 for x in desc), desc
    bb = _restored(blob, len(rows), 32)
    _continue(bb, batch, rows, stops[4], stops[5:], _narrow_same)
    bb.close()


# ---- 6. wide editing documents -------------------------------------------------------------------------
@pytest.mark.parametrize('name', localw.LOGS)
def test_wide_editing_documents_cut_at_every_step(name):
    batch, rows = localw.load(name)
    stops = localw.steps(rows)
    seen = []
    for q in range(len(stops) - 1):
        seen += _through(batch, rows, stops[q], stops[q + 1:], 7, _wide_same)
    assert any('wide' in x['classes'] for x in seen)
    if name == 'localw_offline':
        assert any('wide' in x['classes'] and 'groups' in x['classes'] and x['pending'] > 64 for x in seen), seen


def test_wide_promote_saved_narrow_turns_wide_in_b():
    """localw_promote cut one record before each document's promoting record: a narrow editing document in
    the blob, wide from B's first launch on."""
    batch, rows = localw.load('localw_promote')
    cut = [r['promote']['k'] for r in rows]
    desc = _through(batch, rows, cut, localw.steps(rows), 7, _wide_same)
    assert all('editing' in x['classes'] and 'wide' not in x['classes'] for x in desc), desc
    assert any(x['pending'] > 0 for x in desc)


def test_wide_reconnect_cut_in_the_middle():
    batch, rows = localw.load('localw_reconnect')
    _through_reconnect(batch, rows, 7, _wide_same)


def test_wide_long_document_with_a_big_and_a_wide_row():
    """localw_long at launches of 300 records: the 4096-slot wide editing form, so the document holds a
    big-pool and a wide-pool row when it is saved: its header's flags (csrc/mt_ckpt.h: the word after the 80
    bytes of scalars; MT_CKF_LOC 1, MT_CKF_BIG 2, MT_CKF_WX 8) say so, and the blob holds the wide row's 24
    bytes per segment."""
    batch, rows = localw.load(localw.LONG)
    row = rows[0]
    cut = [row['states'][1][0]]
    blob, desc = _save_at(batch, rows, cut, 300, _wide_same, seg_capacity=8192)
    # (the fixture has no edit pending at any checkpoint of this log -- localw.pending_edits is 0 at all six --
    # so the cut witnesses the rows, not pending groups: those are the other wide logs')
    assert 'wide' in desc[0]['classes'] and 'editing' in desc[0]['classes'], desc
    assert localw.pending_edits(batch, row, cut[0]) == desc[0]['pending'] == 0
    doc = 32 + 16  # (one document: right after the blob header and its one directory entry)
    flags = int(blob[doc + 80:doc + 84].view('<u4')[0])
    assert flags & 1 and flags & 2 and flags & 8 and not flags & 4, flags
    # segments 35 + wide 58 + editing 28 + the wide row 24 bytes each, at the least
    assert desc[0]['bytes'] > 128 + 540 + (35 + 58 + 28 + 24) * desc[0]['nseg'], desc
    bb = _restored(blob, 1, 300)
    _continue(bb, batch, rows, cut, [[row['states'][3][0]], [row['n']]], _wide_same)
    bb.close()


# ---- 7. rows given back and taken again ----------------------------------------------------------------
def test_rows_given_back_and_taken_again():
    from fluidframework_amd import checkpoint
    ob, orows = _log(OFFLINE)
    rb, rrows = _log('local_rounds')
    n_o, n_r, N = len(orows), len(rrows), 32
    assert n_o + n_r <= N

    def all_fine(eng):
        assert [eng.error(s) for s in range(N)] == [(0, 0)] * N

    bb = _engine(N, 32, seg_capacity=4096)
    bb.apply(_place(ob, N, [(i, r['doc'], 0, r['states'][-1][0]) for i, r in enumerate(orows)]))
    all_fine(bb)
    assert 'groups' in checkpoint.describe(bb.save_docs(docs=[0]))[0]['classes']  # (slot 0 holds a group row)
    # local_rounds over those slots
    cut = localw.steps(rrows)[2]
    blob, _ = _save_at(rb, rrows, cut, 32, _narrow_same)
    slots = [n_r - 1 - i for i in range(n_r)]
    bb.restore_docs(blob, docs=np.array(slots, dtype=np.uint32))
    assert np.array_equal(bb.save_docs(docs=slots), blob)
    bb.apply(_place(rb, N, [(slots[i], r['doc'], cut[i], r['states'][-1][0]) for i, r in enumerate(rrows)]))
    all_fine(bb)
    for i, r in enumerate(rrows):
        assert bb.state(slots[i]) == r['states'][-1][1], r['doc']
    # and local_offline, more than 64 edits pending, into the engine's other slots
    cut = localw.steps(orows)[3]
    blob, desc = _save_at(ob, orows, cut, 32, _narrow_same)
    assert any('groups' in x['classes'] for x in desc)
    slots = [N - 1 - i for i in range(n_o)]
    bb.restore_docs(blob, docs=np.array(slots, dtype=np.uint32))
    assert np.array_equal(bb.save_docs(docs=slots), blob)
    bb.apply(_place(ob, N, [(slots[i], r['doc'], cut[i], r['states'][-1][0]) for i, r in enumerate(orows)]))
    all_fine(bb)
    for i, r in enumerate(orows):
        assert bb.state(slots[i]) == r['states'][-1][1], r['doc']
    bb.close()


# ---- 8. one blob, both kinds, a subset -----------------------------------------------------------------
def test_one_blob_of_observers_and_editing_documents_restored_in_part():
    sb, exp = load_golden('scenarios')
    lb, lrows = _log('local_lag')
    n_s, n_l = sb.n_docs, len(lrows)
    N = n_s + n_l
    half, end = np.diff(sb.row_ptr.astype(np.int64)) // 2, np.diff(sb.row_ptr.astype(np.int64))
    cut = localw.steps(lrows)[2]
    a = _engine(N, 7)
    a.apply(_place(sb, N, [(d, d, 0, int(half[d])) for d in range(n_s)]))
    a.apply(_place(lb, N, [(n_s + i, r['doc'], 0, cut[i]) for i, r in enumerate(lrows)]))
    blob = a.save_docs()
    a.close()
    src = list(range(0, N, 2))
    M = len(src)
    slot = {s: M - 1 - j for j, s in enumerate(src)}  # document s of the blob -> B's slot
    bb = _engine(M, 7, seg_capacity=4096)
    bb.restore_docs(blob, docs=[slot[s] for s in src], src=src)
    bb.apply(_place(sb, M, [(slot[s], s, int(half[s]), int(end[s])) for s in src if s < n_s]))
    bb.apply(_place(lb, M, [(slot[s], lrows[s - n_s]['doc'], cut[s - n_s], lrows[s - n_s]['states'][-1][0])
                            for s in src if s >= n_s]))
    cs = bb.checksums()
    assert any(s < n_s for s in src) and any(s >= n_s for s in src)
    for s in src:
        if s < n_s:
            assert '%016x' % cs[slot[s]] == exp[s]['checksum'], s
        else:
            r = lrows[s - n_s]
            assert bb.error(slot[s]) == (0, 0) and bb.state(slot[s]) == r['states'][-1][1], r['doc']
    bb.close()


# ---- 9. refusals that stay -----------------------------------------------------------------------------
def test_refusals_that_stay():
    """An editing document with a reference, and one with declared label keys, are refused by save_docs:
    nothing changes and their editing neighbours still save.  An editing document of 2,200 segments is
    refused by an engine of 2048 (.bad names it), which keeps its own documents as they were.  (No engine
    holds fewer than 2048 segments -- mt_engine_create refuses it -- so local_huge's 1,348 cannot be the
    document that does not fit.)"""
    from fluidframework_amd import checkpoint
    from fluidframework_amd.engine import CheckpointError
    batch, rows = _log('local_lag')
    rows = rows[:4]
    cut = localw.steps(rows)[2]
    a = _engine(4, 7).enable_events(1 << 14)
    a.enable_refs(16)
    a.apply(_span(batch, rows, [0] * 4, cut))
    before = [a.state(i) for i in range(4)]
    assert all(st == r['states'][2][1] for st, r in zip(before, rows))
    assert a.add_refs([0], [0], [0x40])[0] < 16
    a.set_label_keys(0, -1, doc=1)
    for docs in ([0], [1], None):
        with pytest.raises(CheckpointError):
            a.save_docs(docs=docs)
    blob = a.save_docs(docs=[2, 3])
    assert all('editing' in x['classes'] for x in checkpoint.describe(blob))
    assert [a.state(i) for i in range(4)] == before
    a.close()
    # an editing document too large for the target (the smallest engine there is holds 2048 segments, which
    # local_huge's 1,348 fit: test_local_huge's growing document, 2,200 segments, its last edit pending)
    from test_local_huge import _editing_grow_batch
    grow = _editing_grow_batch(2000)
    g = _engine(2, 32, seg_capacity=4096)
    g.apply(_place(grow, 2, [(1, 0, 0, len(grow.ops) - 2)]))
    assert g.error(1) == (0, 0)
    large = g.save_docs()
    g.close()
    desc = checkpoint.describe(large)
    assert desc[1]['nseg'] > 2048 and 'editing' in desc[1]['classes'] and desc[1]['pending'] == 1, desc
    t = _engine(4, 7)
    t.apply(_span(batch, rows, [0] * 4, cut))
    with pytest.raises(CheckpointError) as ei:
        t.restore_docs(large, docs=[0, 1])  # (its first document, empty, fits: the second is named)
    assert ei.value.bad == 1
    assert [t.state(i) for i in range(4)] == before and [t.error(i) for i in range(4)] == [(0, 0)] * 4
    t.restore_docs(blob, docs=[0, 1])  # (and the neighbours' blob restores)
    assert [t.state(0), t.state(1)] == before[2:]
    t.close()


# ---- 10. the committed fixture -------------------------------------------------------------------------
def test_committed_editing_checkpoint_restores_and_continues():
    """tests/golden/checkpoint_v1_editing.bin (the first four local_lag documents at their checkpoint 1, the
    engine's own output, format version 1) restores; the rest of the log then gives the reference's states
    at every later checkpoint."""
    from fluidframework_amd import checkpoint
    blob = checkpoint.read(os.path.join(GOLDEN, 'checkpoint_v1_editing.bin'))
    batch, rows = _log('local_lag')
    rows = rows[:4]
    stops = localw.steps(rows)
    bb = _restored(blob, 4, 7)
    _continue(bb, batch, rows, stops[1], stops[2:], _narrow_same)
    bb.close()
