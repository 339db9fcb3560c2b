"""Document checkpoints on the device (include/mtgpu.h "document checkpoints", DESIGN.md "Checkpoints"):
engine A applies a prefix of a log, saves its documents and is closed; engine B, another object with
another seg_capacity, restores them into its slots in reversed order and applies the rest.

Every expectation is the reference's fixture or the CPU oracle's answer for the whole log, never an
uninterrupted run of the engine: the callbacks B fires after the restore witness the restored heap
and block shape (needsScour, the LRU order), the checksums the segments and the text.
"""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
from test_errors import ref_code
from test_events import LOGS, _err_seqs, _golden_events, _matches

pytestmark = pytest.mark.gpu


def _engine(n, b=0, **kw):
    from fluidframework_amd.engine import MergeEngine
    return MergeEngine(n, ops_per_launch=b, **kw)


def _part(batch, lo, hi, order=None):
    """records [lo[d], hi[d]) of every document d, the documents in `order` (slot s: document order[s])"""
    from fluidframework_amd.oplog import OpBatch
    rp = batch.row_ptr.astype(np.int64)
    order = np.arange(batch.n_docs) if order is None else np.asarray(order)
    rows = [np.arange(rp[d] + lo[d], rp[d] + hi[d]) for d in order]
    cnt = np.array([len(r) for r in rows], dtype=np.int64)
    idx = np.concatenate(rows) if len(rows) else np.zeros(0, np.int64)
    return OpBatch(batch.ops[idx.astype(np.int64)].copy(), batch.payload,
                   np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32))


def _halves(batch):
    n = np.diff(batch.row_ptr.astype(np.int64))
    return n // 2, n


def _through_restore(name, b, events):
    """A: the first half; save; close.  B (seg_capacity 4096, slots reversed): restore, the second half.
    Returns (B, events per document over both engines or None, the blob, B's blob right after the restore)."""
    batch, _ = load_golden(name)
    n = batch.n_docs
    cut, end = _halves(batch)
    rev = np.arange(n)[::-1]
    a = _engine(n, b)
    if events:
        a.enable_events(1 << 16)
    a.apply(_part(batch, 0 * cut, cut))
    ev_a = a.drain_events() if events else None
    blob = a.save_docs()
    a.close()
    bb = _engine(n, b, seg_capacity=4096)
    if events:
        bb.enable_events(1 << 16)
    bb.restore_docs(blob, docs=rev.astype(np.uint32))  # document d of the blob into slot n - 1 - d
    again = bb.save_docs(docs=rev.astype(np.uint32))
    bb.apply(_part(batch, cut, end, order=rev))
    ev = None
    if events:
        ev_b = bb.drain_events()
        ev = [ev_a[d] + ev_b[n - 1 - d] for d in range(n)]
    return bb, ev, blob, again


@pytest.mark.parametrize('b', [0, 3])
@pytest.mark.parametrize('name', LOGS)
def test_observer_documents_continue_with_the_references_callbacks(name, b):
    """(1) and (2): callbacks over both engines = tests/golden/events.jsonl, final checksums and errors =
    the .expected.jsonl ones, and B's own blob right after the restore = A's, byte for byte."""
    from fluidframework_amd import checkpoint
    gold = _golden_events()[name]
    errs = _err_seqs(name)
    _, exp = load_golden(name)
    eng, ev, blob, again = _through_restore(name, b, events=True)
    n = len(exp)
    assert checkpoint.check(blob) == n
    assert np.array_equal(blob, again), (name, b)
    cs = eng.checksums()
    for d in range(n):
        s = n - 1 - d
        assert _matches(gold[d], ev[d], errs.get(d)), (name, d, b)
        assert '%016x' % cs[s] == exp[d]['checksum'], (name, d, b)
        code = ref_code(exp[d]['err']) if exp[d].get('err') else 0
        assert eng.error(s) == ((code, exp[d]['err_seq']) if code else (0, 0)), (name, d, b)
    eng.close()


@pytest.mark.parametrize('name', LOGS + ['wide_many', 'wide_xl'])
def test_observer_documents_without_events(name):
    """The same with events off on both engines (the register engine applies both halves); also the wide
    logs with hundreds of clients and with keys 16..31 (the wide form's extension words)."""
    _, exp = load_golden(name)
    eng, _, blob, again = _through_restore(name, 32, events=False)
    assert np.array_equal(blob, again), name
    cs = eng.checksums()
    n = len(exp)
    for d in range(n):
        assert '%016x' % cs[n - 1 - d] == exp[d]['checksum'], (name, d)
        code = ref_code(exp[d]['err']) if exp[d].get('err') else 0
        assert eng.error(n - 1 - d) == ((code, exp[d]['err_seq']) if code else (0, 0)), (name, d)
    eng.close()


# ---- (3) tails -----------------------------------------------------------------------------------
TAIL_NSEG = [0, 1, 63, 64, 65, 127, 128, 129, 1023]


def _tail_log(first_client):
    """One document per TAIL_NSEG of single-character inserts at position 0 by three clients (nothing
    coalesces: the MSN stays 0), then 16 documents of three inserts whose text lengths leave text_top at
    every residue mod 16."""
    from fluidframework_amd.oplog import INSERT, OP_DTYPE, OpBatch
    recs, payload, rp = [], bytearray(), [0]

    def ins(k, text):
        recs.append((k + 1, k, 0, first_client + k % 3, INSERT, 0, 0, 0, len(payload), len(text)))
        payload.extend(text)

    for ns in TAIL_NSEG:
        for k in range(ns):
            ins(k, b'abcdefghijklmnopqrstuvwxyz'[k % 26:k % 26 + 1])
        rp.append(len(recs))
    for r in range(16):
        for k, ln in enumerate((7, 9 + r, 16)):
            ins(k, bytes(65 + (k + q) % 26 for q in range(ln)))
        rp.append(len(recs))
    return OpBatch(np.array(recs, dtype=OP_DTYPE), np.frombuffer(bytes(payload), np.uint8), np.array(rp, np.uint32))


@pytest.mark.parametrize('wide', [False, True])
def test_tails_of_every_section(oracle_lib, wide):
    """Segment counts around the 64-lane and 16-byte vector boundaries, text tops at every residue mod 16
    (a wide document: odd UTF-16 unit counts among them).  The restored state is the CPU oracle's; the
    wide documents' (client ids from 64: the wide form) is oracle/canon.py's checksum of the same state
    with those client ids."""
    from oracle import canon
    narrow = _tail_log(1)
    o = oracle_lib.Oracle(narrow.n_docs).apply(narrow)
    if wide:
        want = []
        for d in range(narrow.n_docs):
            st = o.state(d)
            st = json.loads(st) if isinstance(st, (str, bytes)) else st
            for sg in st['segs']:
                sg[2] += 63
            want.append(canon.checksum(st))
        want = np.array(want, dtype=np.uint64)
        batch = _tail_log(64)
    else:
        want, batch = o.checksums(), narrow
    n = batch.n_docs
    a = _engine(n, 32)
    a.apply(batch)
    blob = a.save_docs()
    a.close()
    from fluidframework_amd import checkpoint
    desc = checkpoint.describe(blob)
    assert [r['nseg'] for r in desc[:len(TAIL_NSEG)]] == TAIL_NSEG
    assert sorted({r['text_units'] % 16 for r in desc}) == list(range(16))
    assert all(('wide' in r['classes']) == wide for r in desc if r['nseg'])
    bb = _engine(n, 32, seg_capacity=4096)
    rev = np.arange(n, dtype=np.uint32)[::-1].copy()
    bb.restore_docs(blob, docs=rev)
    assert np.array_equal(bb.checksums()[::-1], want)
    assert np.array_equal(bb.save_docs(docs=rev), blob)
    bb.close()


# ---- (7) refusals: nothing moves -----------------------------------------------------------------
def _large_log():
    """the log of test_events.test_engine_events_large_document: 2,600 segments"""
    from fluidframework_amd.oplog import INSERT, NOOP, OP_DTYPE, REMOVE, OpBatch
    recs, payload = [], bytearray()
    for k in range(2600):
        recs.append((k + 1, k, 0, 1 + k % 3, INSERT, 0, k % 17, 0, len(payload), 1))
        payload += b'abcdefghij'[k % 10:k % 10 + 1]
    recs.append((2601, 2600, 0, 2, REMOVE, 0, 100, 900, 0, 0))
    recs.append((2602, 2601, 2601, 1, NOOP, 0, 0, 0, 0, 0))
    return OpBatch(np.array(recs, dtype=OP_DTYPE), np.frombuffer(bytes(payload), np.uint8),
                   np.array([0, len(recs)], np.uint32))


def test_refusals_touch_nothing(oracle_lib):
    from fluidframework_amd import checkpoint
    from fluidframework_amd.engine import CheckpointError
    big = _large_log()
    a = _engine(1, 64, seg_capacity=4096)
    a.apply(big)
    assert a.error(0) == (0, 0)
    blob = a.save_docs()
    assert checkpoint.describe(blob)[0]['nseg'] > 2048
    # the large document restores where it fits, and is the oracle's
    c = _engine(1, 64, seg_capacity=4096)
    c.restore_docs(blob)
    assert c.checksums()[0] == oracle_lib.Oracle(1).apply(big).checksums()[0]
    c.close()
    a.close()
    # a 2048 engine with documents of its own (the `errors` log: halted documents among them)
    batch, exp = load_golden('errors')
    t = _engine(batch.n_docs, 7)
    t.apply(batch)
    before = (t.checksums().copy(), [t.error(d) for d in range(batch.n_docs)])

    def unchanged():
        return np.array_equal(t.checksums(), before[0]) and [t.error(d) for d in range(batch.n_docs)] == before[1]

    with pytest.raises(CheckpointError) as ei:
        t.restore_docs(blob, docs=[1])
    assert ei.value.bad == 0 and unchanged()
    # one flipped byte: refused by the host check, before anything reaches the device
    own = t.save_docs()
    flipped = own.copy()
    flipped[len(flipped) // 2] ^= 0x10
    with pytest.raises(CheckpointError) as ei:
        t.restore_docs(flipped)
    assert ei.value.bad == 0xFFFFFFFF and unchanged()
    # and two documents into one slot, or a document the blob does not have: a bad argument
    from fluidframework_amd.engine import MtError
    with pytest.raises(MtError):
        t.restore_docs(own, docs=[0, 0], src=[0, 1])
    with pytest.raises(MtError):
        t.restore_docs(own, docs=[0], src=[batch.n_docs])
    assert unchanged()
    t.close()


def test_documents_past_observers_are_refused():
    """Save and restore admit observer documents today (include/mtgpu.h): a document with references or
    with declared label keys is refused by save_docs, nothing is written, and its neighbours still save."""
    from fluidframework_amd import checkpoint
    from fluidframework_amd.engine import CheckpointError
    batch, _ = load_golden('scenarios')
    a = _engine(batch.n_docs, 7).enable_events(1 << 14)
    a.enable_refs(16)
    a.apply(batch)
    before = a.checksums().copy()
    a.add_refs([0, 0], [0, 1], [0x40, 0x40])
    a.set_label_keys(0, -1, doc=1)
    for docs in ([0], [1], None):
        with pytest.raises(CheckpointError):
            a.save_docs(docs=docs)
    blob = a.save_docs(docs=[2, 3])
    assert checkpoint.check(blob) == 2 and np.array_equal(a.checksums(), before)
    t = _engine(2, 7)
    t.restore_docs(blob)
    assert np.array_equal(t.checksums(), before[2:4])
    a.close()
    t.close()


# ---- more than one workgroup per document ----------------------------------------------------------
def test_a_document_past_128_kib_is_copied_by_several_workgroups(oracle_lib):
    """4,500 inserts leave several thousand segments, more than 128 KiB of blob: pack and unpack run
    several workgroups on the document (one per 64 KiB).  The restored document is the CPU oracle's,
    and saves to the same bytes."""
    from fluidframework_amd import checkpoint
    from fluidframework_amd.oplog import INSERT, OP_DTYPE, OpBatch
    recs, payload = [], bytearray()
    for k in range(4500):
        recs.append((k + 1, k, 0, 1 + k % 3, INSERT, 0, k % 29, 0, len(payload), 1 + k % 2))
        payload += b'abcdefghijk'[k % 10:k % 10 + 1 + k % 2]
    batch = OpBatch(np.array(recs, dtype=OP_DTYPE), np.frombuffer(bytes(payload), np.uint8),
                    np.array([0, len(recs)], np.uint32))
    o = oracle_lib.Oracle(1).apply(batch)
    want = o.checksums()[0]
    a = _engine(3, 64, seg_capacity=8192)
    a.apply(OpBatch(batch.ops, batch.payload, np.array([0, 0, len(recs), len(recs)], np.uint32)))  # slot 1
    assert a.error(1) == (0, 0)
    blob = a.save_docs(docs=[1])
    a.close()
    d = checkpoint.describe(blob)[0]
    assert d['nseg'] == o.nsegs(0) >= 4500 and d['bytes'] >= 2 << 16
    bb = _engine(2, 64, seg_capacity=8192)
    bb.restore_docs(blob, docs=[1])
    assert bb.checksums()[1] == want and bb.error(1) == (0, 0)
    assert np.array_equal(bb.save_docs(docs=[1]), blob)
    assert bb.checkpoint_stats()[1] == len(blob) - 48 and bb.checkpoint_stats()[3] == len(blob) - 48
    bb.close()


# ---- (8) reshard ---------------------------------------------------------------------------------
def test_reshard_two_ranks_to_three():
    """synth_c3 over two engines by shard.route, the first half applied, shard.moves(ids, 2, 3) carried out
    with save / restore (the src subset argument) into three engines, the second half applied: the XOR
    digest of all checksums is the digest of the fixture's."""
    from fluidframework_amd import shard
    batch, exp = load_golden('synth_c3')
    n = batch.n_docs
    ids = np.arange(n, dtype=np.uint64)
    cut, end = _halves(batch)
    old = [np.flatnonzero(shard.route(ids, 2) == r) for r in range(2)]
    new = [np.flatnonzero(shard.route(ids, 3) == r) for r in range(3)]
    engines = []
    for docs in old:
        e = _engine(len(docs), 32)
        e.apply(_part(batch, 0 * cut, cut, order=docs))
        engines.append(e)
    moved, src_rank, dst_rank = shard.moves(ids, 2, 3)
    assert all(shard.route(ids, 3)[int(d)] == t for d, t in zip(moved, dst_rank))
    # each old rank saves everything it holds once; each new rank takes its documents out of those blobs
    blobs = [e.save_docs() for e in engines]
    for e in engines:
        e.close()
    cs = np.zeros(n, dtype=np.uint64)
    for r, docs in enumerate(new):
        e = _engine(len(docs), 32, seg_capacity=4096)
        slot = {int(d): s for s, d in enumerate(docs)}
        for q in range(2):  # the documents that come from old rank q: stayed (q == r) or moved
            mine = [int(d) for d in docs if shard.route(ids, 2)[int(d)] == q]
            if not mine:
                continue
            where = {int(d): s for s, d in enumerate(old[q])}
            e.restore_docs(blobs[q], docs=[slot[d] for d in mine], src=[where[d] for d in mine])
        e.apply(_part(batch, cut, end, order=docs))
        cs[docs] = e.checksums()
        e.close()
    assert set(int(d) for d in moved) == {int(d) for d in ids if shard.route(ids, 2)[int(d)] != shard.route(ids, 3)[int(d)]}
    want = np.array([int(r['checksum'], 16) for r in exp], dtype=np.uint64)
    assert shard.digest(cs) == shard.digest(want)
    assert np.array_equal(cs, want)


# ---- the committed fixture -------------------------------------------------------------------------
def test_committed_checkpoint_restores_and_continues():
    """tests/golden/checkpoint_v1.bin (the `scenarios` documents at half their records, format version 1)
    restores, and the second half then gives the golden checksums and, with the first half's callbacks
    from the fixture's own log prefix, the golden events' tail."""
    from fluidframework_amd import checkpoint
    blob = checkpoint.read(os.path.join(GOLDEN, 'checkpoint_v1.bin'))
    batch, exp = load_golden('scenarios')
    gold = _golden_events()['scenarios']
    cut, end = _halves(batch)
    e = _engine(batch.n_docs, 3).enable_events(1 << 16)
    e.restore_docs(blob)
    e.apply(_part(batch, cut, end))
    ev = e.drain_events()
    cs = e.checksums()
    for d in range(batch.n_docs):
        assert '%016x' % cs[d] == exp[d]['checksum'], d
        first_seq = int(batch.ops[int(batch.row_ptr[d]) + int(cut[d])]['seq']) if end[d] > cut[d] else 1 << 30
        assert ev[d] == [c for c in gold[d]['events'] if c[0] >= first_seq], d
    e.close()
