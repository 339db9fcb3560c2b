"""Marker-relative op records on the device (include/mtgpu.h "marker-relative positions", "marker ids"):
the engine fed the relative records of tests/golden/relpos*.mtlog -- a farm of reference Clients whose
annotateMarker ops every receiver resolves (tests/golden/relpos_ref.js) -- against the reference's
states and callbacks, against itself fed relpos.lower()'s absolute log, and mt_marker_positions against
the reference's posFromRelativePos answers."""
import numpy as np
import pytest

from test_relpos import LOGS, MARKER_KEY, fixture, load_log, lowered

pytestmark = pytest.mark.gpu

CLASS_LDS, CLASS_MASK = 0x20000000, 0x7C000000
EVCAP = 1 << 14


def pieces(batch, ks):
    """The batch cut at the record counts ks (ascending): one OpBatch per piece, every document's
    records [previous k, k)."""
    from fluidframework_amd.oplog import OpBatch
    out, done = [], [0] * batch.n_docs
    for k in ks:
        idx, rp = [], [0]
        for d in range(batch.n_docs):
            a, e = int(batch.row_ptr[d]), int(batch.row_ptr[d + 1])
            hi = min(k, e - a)
            idx.extend(range(a + done[d], a + hi))
            rp.append(len(idx))
            done[d] = max(done[d], hi)
        out.append(OpBatch(batch.ops[idx], batch.payload, np.array(rp, np.uint32)))
    return out


@pytest.mark.parametrize('b', [1, 7, 32])
@pytest.mark.parametrize('name', LOGS)
def test_engine_replays_relative_records(oracle_lib, name, b):
    """The narrow log (the LDS engine at register capacities), the wide log (the wide form) and the
    editing client's log (the editing form, edits pending around the markers): the reference's state at
    every checkpoint (its canonical checksum; the state itself where the fixture keeps it), its callbacks
    (their count and digest), and the checksums of the engine fed the lowered log."""
    import sys
    from test_relpos import GOLDEN
    sys.path.insert(0, GOLDEN)
    from make_relpos import digest
    from fluidframework_amd.engine import MergeEngine
    _, by_log = fixture()
    rows = by_log[name]
    batch = load_log(name)
    ks = sorted(set(c['k'] for r in rows for c in r['checkpoints']))
    eng = MergeEngine(batch.n_docs, ops_per_launch=b).enable_events(EVCAP)
    events = [[] for _ in rows]
    for k, piece in zip(ks, pieces(batch, ks)):
        eng.apply(piece)
        for d, ev in enumerate(eng.drain_events()):
            events[d].extend(ev)
        cs = eng.checksums()
        for r in rows:
            assert eng.error(r['doc']) == (0, 0), (name, r['doc'], k, eng.error(r['doc']))
            for c in r['checkpoints']:
                if c['k'] == k:
                    assert '%016x' % int(cs[r['doc']]) == c['checksum'], (name, r['doc'], k, b)
                    if 'state' in c:
                        assert eng.state(r['doc']) == c['state'], (name, r['doc'], k, b)
    for r in rows:
        assert len(events[r['doc']]) == r['events']['n'], (name, r['doc'], b)
        assert digest(events[r['doc']]) == r['events']['sha256'], (name, r['doc'], b)
    got = eng.checksums()
    eng.close()
    low, _, _ = lowered(name, oracle_lib)
    ref = MergeEngine(low.n_docs, ops_per_launch=b)
    ref.apply(low)
    want = ref.checksums()
    ref.close()
    assert [int(x) for x in got] == [int(x) for x in want]


def tiled(batch, d, k):
    """Document d of a relative log behind k one-unit segments (inserted first, at position 0, by three
    clients in turn): its sequence numbers moved up by k, its absolute positions by the k units in front,
    and every msn 0, so that zamboni never packs the document below the workspace classes."""
    from fluidframework_amd.oplog import INSERT, OP_DTYPE, OP_REL1, OP_REL2, NOOP, OpBatch, base_type
    a, e = int(batch.row_ptr[d]), int(batch.row_ptr[d + 1])
    pre = np.zeros(k, dtype=OP_DTYPE)
    pre['seq'] = np.arange(1, k + 1)
    pre['ref_seq'] = np.arange(0, k)
    pre['client'] = 1 + np.arange(k) % 3
    pre['type'] = INSERT
    pre['payload_off'] = len(batch.payload) + np.arange(k) % 10
    pre['payload_len'] = 1
    ops = batch.ops[a:e].copy()
    ops['seq'] += k
    ops['ref_seq'] += k
    ops['msn'] = 0
    for o in ops:
        t = int(o['type'])
        if base_type(t) == NOOP:
            continue
        if not t & OP_REL1:
            o['pos1'] += k
        if base_type(t) != INSERT and not t & OP_REL2:
            o['pos2'] += k
    payload = np.concatenate([batch.payload, np.frombuffer(b'abcdefghij', np.uint8)])
    return OpBatch(np.concatenate([pre, ops]), payload, np.array([0, k + e - a], np.uint32))


def test_workspace_form_document(oracle_lib):
    """A document past 2048 segments (the HBM-workspace form): the markers lie behind 2300 leaves."""
    from fluidframework_amd import relpos
    from fluidframework_amd.engine import MergeEngine
    from fluidframework_amd.oplog import OP_REL
    batch = tiled(load_log('relpos'), 0, 2300)
    o = oracle_lib.Oracle(1)
    low, res = relpos.lower(batch, o)
    assert o.error(0) == (0, 0) and o.nsegs(0) > 2600 and len(res) > 100
    assert sum(1 for x in res if x[4] == 0 and x[2] > 2300) > 100   # resolved, behind the tiled leaves
    eng = MergeEngine(1, ops_per_launch=32, seg_capacity=4096)
    eng.apply(batch)
    assert eng.error(0) == (0, 0)
    assert int(eng.seg_counts()[0]) == o.nsegs(0)
    assert int(eng.checksums()[0]) == int(o.checksums()[0])
    assert eng.state(0) == o.state(0)
    used = {cap for cap, _, launches, _ in eng.last_class_stats() if launches}
    assert any(not c & CLASS_MASK and c >= 2048 for c in used), used
    # and the engine fed the lowered log
    eng2 = MergeEngine(1, ops_per_launch=32, seg_capacity=4096)
    eng2.apply(low)
    assert int(eng2.checksums()[0]) == int(eng.checksums()[0]) and not (low.ops['type'] & OP_REL).any()
    eng.close()
    eng2.close()


def small_doc():
    """'abcdef', a marker with id 5 (key 3) at 3, 'gh' at the end; then one launch of eight records that
    mixes relative and absolute ops, then sixteen absolute ones."""
    from fluidframework_amd.oplog import ANNOTATE, F_MARKER, INSERT, REMOVE
    rb, ra = dict(key=3, value=5, before=True), dict(key=3, value=5)
    recs = [(1, 0, 0, 1, INSERT, 0, 0, 'abcdef', None, 0), (2, 1, 0, 2, INSERT, 3, 0, '\x01', {3: 5}, F_MARKER),
            (3, 2, 0, 1, INSERT, 7, 0, 'gh', None, 0), (4, 3, 0, 2, INSERT, 0, 0, 'Q', None, 0),
            (5, 4, 0, 1, INSERT, 1, 0, 'R', None, 0), (6, 5, 0, 2, REMOVE, 0, 1, None, None, 0),
            (7, 6, 0, 1, INSERT, 0, 0, 'S', None, 0), (8, 7, 0, 2, INSERT, 0, 0, 'T', None, 0)]
    mixed = [(9, 8, 0, 1, INSERT, 2, 0, 'xy', None, 0), (10, 8, 0, 2, ANNOTATE, 0, 0, None, {1: 2}, 0, rb, ra),
             (11, 9, 0, 1, REMOVE, 0, 1, None, None, 0), (12, 11, 0, 2, INSERT, 0, 0, 'in', None, 0, ra, None),
             (13, 12, 0, 1, ANNOTATE, 1, 3, None, {2: 1}, 0),
             (14, 12, 0, 2, REMOVE, 0, 0, None, None, 0, dict(key=3, value=5, before=True, offset=1), ra),
             (15, 14, 0, 1, INSERT, 0, 0, 'U', None, 0), (16, 15, 0, 2, INSERT, 1, 0, 'V', None, 0)]
    after = [(17 + i, 16 + i, 0, 1 + i % 2, INSERT, i % 3, 0, 'w', None, 0) for i in range(16)]
    return recs, mixed, after


def test_mixed_launch_then_back_to_the_register_engine(oracle_lib):
    """A launch that mixes relative and absolute ops runs on the LDS engine at the document's register
    class's capacity, for that launch only: the launches before and after it run on the register engine.
    End state and checksum are those of the lowered run."""
    from fluidframework_amd import relpos
    from fluidframework_amd.engine import MergeEngine
    from fluidframework_amd.oplog import build_batch
    recs, mixed, after = small_doc()
    whole = build_batch([recs + mixed + after])
    o = oracle_lib.Oracle(1)
    low, res = relpos.lower(whole, o)
    # record 9's sender (client 2 at refSeq 8) has not seen 'xy': "TSRabc|defgh", the marker at 6
    assert [(i, p1, p2) for _, i, p1, p2, _ in res] == [(9, 6, 7), (11, 8, 0), (13, 6, 8)]
    assert o.error(0) == (0, 0)
    eng = MergeEngine(1, ops_per_launch=8)
    used = []
    for part in pieces(whole, [8, 16, 24, 32]):
        eng.apply(part)
        used.append({cap for cap, _, launches, _ in eng.last_class_stats() if launches})
    assert eng.error(0) == (0, 0)
    assert all(not c & CLASS_MASK and c <= 1024 for c in used[0]), used
    assert all(c & CLASS_LDS for c in used[1]) and used[1], used
    assert all(not c & CLASS_MASK and c <= 1024 for c in used[2] | used[3]) and used[2] and used[3], used
    assert eng.state(0) == o.state(0) and int(eng.checksums()[0]) == int(o.checksums()[0])
    eng.close()
    eng = MergeEngine(1, ops_per_launch=8)
    eng.apply(low)
    assert int(eng.checksums()[0]) == int(o.checksums()[0])
    eng.close()


@pytest.mark.parametrize('form', ['host', 'device'])
@pytest.mark.parametrize('name', LOGS)
def test_marker_positions_against_the_reference(name, form):
    """mt_marker_positions at the fixture's checkpoints: Client.posFromRelativePos in the local view and
    MergeTree.posFromRelativePos in remote views, formed from the kernel's (position, length)."""
    from fluidframework_amd.engine import MARKER_QUERY_DTYPE, MARKER_RESULT_DTYPE, POS_LOCAL, MergeEngine
    from fluidframework_amd.hipmem import DeviceBuffer
    from fluidframework_amd.relpos import position_of
    _, by_log = fixture()
    rows = by_log[name]
    batch = load_log(name)
    ks = sorted(set(c['k'] for r in rows for c in r['checkpoints']))
    eng = MergeEngine(batch.n_docs, ops_per_launch=32)
    checked = 0
    for k, piece in zip(ks, pieces(batch, ks)):
        eng.apply(piece)
        qs = [(r['doc'], q) for r in rows for q in r['pfr'] if q[0] == k]
        if not qs:
            continue
        arr = np.zeros(len(qs), dtype=MARKER_QUERY_DTYPE)
        for i, (d, (_, view, value, _, _, _)) in enumerate(qs):
            arr[i] = (d, POS_LOCAL if view is None else view[0], 0 if view is None else view[1], MARKER_KEY[name], 0,
                      value, 0)
        if form == 'host':
            got = eng.marker_positions(arr)
        else:
            dq, dr = DeviceBuffer(arr.nbytes).upload(arr), DeviceBuffer(len(arr) * MARKER_RESULT_DTYPE.itemsize)
            eng.marker_positions_device(dq.ptr, len(arr), dr.ptr)
            got = dr.download(MARKER_RESULT_DTYPE)
        for g, (d, (_, view, value, before, offset, want)) in zip(got, qs):
            ans = -1 if int(g['ordinal']) < 0 else position_of(int(g['position']), int(g['length']), before, offset or 0)
            assert ans == want, (name, d, k, view, value, before, offset)
            checked += 1
    eng.close()
    assert checked > 20


def test_marker_positions_edge_shapes(oracle_lib):
    """Small hand-built documents: the marker at ordinal 0, 63, 64 and last; behind a long removed run; a
    document with no markers; value id 0; a document with a sticky error."""
    from fluidframework_amd.engine import (MARKER_QUERY_DTYPE, MKF_HIDDEN, MKF_TOMBSTONE, POS_LOCAL, MergeEngine)
    from fluidframework_amd.oplog import F_MARKER, INSERT, REMOVE, build_batch
    from fluidframework_amd.relpos import choose_marker, marker_position

    def leaves(n, marks):
        """n one-unit leaves appended in order by alternating clients (msn 0: none is packed); marks:
        {ordinal: value id} of the leaves that are markers with that id under key 2"""
        return [(i + 1, i, 0, 1 + i % 2, INSERT, i, 0, '\x01' if i in marks else 'abcdefghij'[i % 10],
                 {2: marks[i]} if i in marks else None, F_MARKER if i in marks else 0) for i in range(n)]
    docs = [leaves(130, {0: 1, 63: 2, 64: 3, 129: 4}),
            # leaves 10..99 removed by client 2 at seq 141, the marker (id 7) at ordinal 100
            leaves(140, {100: 7}) + [(141, 140, 0, 2, REMOVE, 10, 100, None, None, 0)],
            leaves(70, {}),
            # a sticky error: the last record is refused (negative position), the state stays
            leaves(66, {65: 9}) + [(67, 66, 0, 1, REMOVE, -3, 2, None, None, 0)]]
    batch = build_batch(docs)
    o = oracle_lib.Oracle(4).apply(batch)
    eng = MergeEngine(4, ops_per_launch=32)
    eng.apply(batch)
    assert eng.error(3)[0] == 7 and [eng.error(d)[0] for d in range(3)] == [0, 0, 0]
    q = [(0, POS_LOCAL, 0, 2, 0, 1, 0), (0, POS_LOCAL, 0, 2, 0, 2, 0), (0, POS_LOCAL, 0, 2, 0, 3, 0),
         (0, POS_LOCAL, 0, 2, 0, 4, 0), (0, 64, 2, 2, 0, 3, 0), (0, 63, 1, 2, 0, 4, 0),
         (1, POS_LOCAL, 0, 2, 0, 7, 0), (1, 140, 1, 2, 0, 7, 0), (1, 141, 1, 2, 0, 7, 0), (1, 50, 2, 2, 0, 7, 0),
         (2, POS_LOCAL, 0, 2, 0, 1, 0), (0, POS_LOCAL, 0, 2, 0, 0, 0), (0, POS_LOCAL, 0, 3, 0, 1, 0),
         (0, POS_LOCAL, 0, 31, 0, 1, 0), (3, POS_LOCAL, 0, 2, 0, 9, 0)]
    got = eng.marker_positions(np.array(q, dtype=MARKER_QUERY_DTYPE))
    for g, (d, ref_seq, client, key, _, value, _) in zip(got, q):
        st = o.state(d)
        k = choose_marker(st, key, value)
        view = () if ref_seq == POS_LOCAL else (ref_seq, client)
        if k is None:
            assert (int(g['ordinal']), int(g['position']), int(g['length'])) == (-1, 0, 0), (d, value)
        else:
            assert (int(g['ordinal']), int(g['position']), int(g['length'])) == (k, marker_position(st, k, *view), 1)
    assert [int(g['ordinal']) for g in got] == [0, 63, 64, 129, 64, 129, 100, 100, 100, 100, -1, -1, -1, -1, 65]
    # behind the removed run: 10 units in the local view and for anyone who saw the removal, 100 before it;
    # client 2 at refSeq 50 has seen 51 leaves and its own removal: 10 units, and not the marker
    assert [int(g['position']) for g in got[6:10]] == [10, 100, 10, 10]
    assert int(got[9]['flags']) & MKF_HIDDEN and not int(got[9]['flags']) & MKF_TOMBSTONE
    assert int(got[6]['flags']) == 0
    # client 1 at refSeq 63 has not seen leaf 129 (seq 130, client 2's): hidden in that view, its prefix
    # what the view shows -- the 63 leaves up to seq 63 and client 1's own 33 later ones
    assert int(got[5]['flags']) == MKF_HIDDEN and int(got[5]['position']) == 96
    eng.close()


def test_tombstone_flag_and_removed_marker():
    from fluidframework_amd.engine import MARKER_QUERY_DTYPE, MKF_HIDDEN, MKF_TOMBSTONE, POS_LOCAL, MergeEngine
    from fluidframework_amd.oplog import F_MARKER, INSERT, REMOVE, build_batch
    batch = build_batch([[(1, 0, 0, 1, INSERT, 0, 0, 'abcd', None, 0), (2, 1, 0, 2, INSERT, 2, 0, '\x01', {1: 4}, F_MARKER),
                          (3, 2, 0, 1, REMOVE, 2, 3, None, None, 0)]])
    eng = MergeEngine(1, ops_per_launch=32)
    eng.apply(batch)
    got = eng.marker_positions(np.array([(0, POS_LOCAL, 0, 1, 0, 4, 0), (0, 2, 2, 1, 0, 4, 0)], dtype=MARKER_QUERY_DTYPE))
    assert [(int(g['ordinal']), int(g['position']), int(g['flags'])) for g in got] == \
        [(1, 2, MKF_HIDDEN | MKF_TOMBSTONE), (1, 2, MKF_TOMBSTONE)]
    eng.close()


def test_error_cases():
    """MT_DERR_BAD_OP (7) at the record's seq, the document halted in the state before it: a relative
    local record, a resolved negative position, an unresolved insert, one unresolved end beside an
    absolute one, a payload shorter than its tail.  A relative range whose two ids name nothing is no error."""
    from fluidframework_amd.engine import MergeEngine, MtError
    from fluidframework_amd.oplog import ANNOTATE, F_MARKER, INSERT, REMOVE, OpBatch, build_batch
    base = [(1, 0, 0, 1, INSERT, 0, 0, 'abcdef', None, 0), (2, 1, 0, 2, INSERT, 1, 0, '\x01', {3: 5}, F_MARKER)]
    rb, ra = dict(key=3, value=5, before=True), dict(key=3, value=5)
    ub, ua = dict(key=3, value=6, before=True), dict(key=3, value=6)
    bad = [(-1, 0, 0, 1, ANNOTATE, 0, 0, None, {1: 1}, 0, rb, ra),                                  # a relative local record
           (3, 2, 0, 1, REMOVE, 0, 0, None, None, 0, dict(key=3, value=5, before=True, offset=2), ra),  # 1 - 2 < 0
           (3, 2, 0, 1, INSERT, 0, 0, 'zz', None, 0, ua, None),                                    # an unresolved insert
           (3, 2, 0, 1, REMOVE, 0, 3, None, None, 0, ub, None),                                    # one unresolved end
           (3, 2, 0, 1, ANNOTATE, 0, 0, None, {1: 1}, 0, rb, ra)]                                  # (cut short below)
    ok = (3, 2, 0, 1, ANNOTATE, 0, 0, None, {1: 1}, 0, ub, ua)
    batch = build_batch([base + [r] for r in bad] + [base + [ok]] + [base])
    ops = batch.ops.copy()
    ops[int(batch.row_ptr[5]) - 1]['payload_len'] -= 8    # the tail needs 2 + 16 bytes, the record holds 10
    batch = OpBatch(ops, batch.payload, batch.row_ptr)
    eng = MergeEngine(batch.n_docs, ops_per_launch=32)
    eng.apply(batch)
    want = eng.state(6)
    assert [eng.error(d) for d in range(7)] == [(7, -1), (7, 3), (7, 3), (7, 3), (7, 3), (0, 0), (0, 0)]
    for d in range(5):
        assert eng.state(d) == want, d
    assert eng.state(5)['segs'] == want['segs'] and eng.state(5)['seq'] == 3
    eng.close()
    # a payload that ends past the batch's bytes is refused at the door, tail blocks included
    ops = build_batch([base + [ok]]).ops.copy()
    short = OpBatch(ops, build_batch([base + [ok]]).payload[:-4], np.array([0, 3], np.uint32))
    eng = MergeEngine(1, ops_per_launch=32)
    with pytest.raises(MtError):
        eng.apply(short)
    eng.close()
