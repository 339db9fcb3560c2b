"""Device position queries (include/mtgpu.h mt_resolve_positions; SURVEY.md §8(b) read surface):
MergeTree.getContainingSegment(pos, refSeq, clientId) (mergeTree.ts:1623-1634 through searchBlock,
:1797-1829) and getPosition (mergeTree.ts:1585-1602) answered by one wave per query over the state in
HBM, checked against the same questions asked of the reference's own final states
(tests/golden/*.expected.jsonl, produced by the transpiled reference): every position of the local
view and of remote clients' views at two refSeqs, past-the-end and negative positions, and every
ordinal.  The restatement here is searchBlock's walk flattened over the leaves in order (a block is
entered iff the first leaf that holds pos is inside it)."""
import numpy as np
import pytest

from conftest import WIDE_SETS, load_golden
from view_docs import expected as _expected, high_members, units as _units, view_len as _view_len

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', ['scenarios', 'markers', 'synth_c3', 'synth_c4', 'synth_tiny'] + WIDE_SETS)
def test_resolve_positions_match_reference_states(name):
    from fluidframework_amd.engine import POS_CONTAINING, POS_LOCAL, POS_OF_ORDINAL, POS_QUERY_DTYPE, MergeEngine
    batch, exp = load_golden(name)
    eng = MergeEngine(batch.n_docs, ops_per_launch=32)
    eng.apply(batch)
    rows, want = [], []
    high_views = 0
    for r in exp:
        d, st = r['doc'], r['state']
        if eng.error(d) != (0, 0):
            continue
        inserters = sorted({s[2] for s in st['segs'] if s[2] > 0})
        clients = inserters[:3]
        # and where the state has them: the highest inserter, a removedClient and up to three overlap
        # members >= 64 (in a wide document these read the overlap list and the ids' high bytes)
        removed = [s for s in st['segs'] if s[4] > 0]
        extra = inserters[-1:] + [s[4] for s in removed[:1]] + sorted({m for s in removed for m in high_members(s[5])})[-3:]
        extra = [c for c in dict.fromkeys(extra) if c not in clients]
        high_views += sum(1 for c in extra if c >= 64)
        views = [(None, 0)] + [(rs, c) for c in clients + extra for rs in (st['msn'], st['seq'])]
        for ref_seq, client in views:
            vlen = sum(_view_len(s, ref_seq, client) for s in st['segs'])
            stride = max(1, (vlen + 2) // 24)
            for p in sorted(set(list(range(-1, vlen + 2, stride)) + [vlen, vlen + 1])):
                rows.append((d, p, POS_LOCAL if ref_seq is None else ref_seq, client, POS_CONTAINING))
                want.append(_expected(st, p, ref_seq, client))
        n = len(st['segs'])
        lp = 0
        for i, s in enumerate(st['segs']):
            rows.append((d, i, POS_LOCAL, 0, POS_OF_ORDINAL))
            want.append((i, 0, lp, _units(s[0])))
            lp += _view_len(s, None, 0)
        rows.append((d, n, POS_LOCAL, 0, POS_OF_ORDINAL))
        want.append((-1, None, None, None))
        for c in extra:   # getPosition is the local view's whoever asks
            lp = 0
            for i, s in enumerate(st['segs']):
                rows.append((d, i, st['seq'], c, POS_OF_ORDINAL))
                want.append((i, 0, lp, _units(s[0])))
                lp += _view_len(s, None, 0)
            rows.append((d, n, st['msn'], c, POS_OF_ORDINAL))
            want.append((-1, None, None, None))
    q = np.array(rows, dtype=POS_QUERY_DTYPE)
    got = eng.resolve_positions(q)
    for k, (g, w) in enumerate(zip(got, want)):
        if w[1] is None:  # an ordinal past the end: none
            ok = int(g['ordinal']) == -1
        elif w[0] < 0:  # past the view: none, with the view's overshoot and the local length
            ok = int(g['ordinal']) == -1 and int(g['offset']) == w[1] and int(g['position']) == w[2]
        else:
            ok = (int(g['ordinal']), int(g['offset']), int(g['position']), int(g['length'])) == w
        if not ok:
            pytest.fail(f'{name}: query {rows[k]} -> {tuple(int(x) for x in g)}, reference state gives {w}')
    assert len(rows) > 100
    assert high_views > 0 or name not in WIDE_SETS


def test_resolve_positions_on_editing_documents():
    """The local view of an editing client counts its pending inserts and hides its pending
    removals: getContainingSegment over every position of the local_rounds / local_lag documents at
    their final states (the reference's canonical states, tests/golden/local.expected.jsonl)."""
    import json
    import os

    from conftest import GOLDEN
    from fluidframework_amd.engine import POS_CONTAINING, POS_LOCAL, POS_QUERY_DTYPE, MergeEngine
    from fluidframework_amd.oplog import OpBatch
    with open(os.path.join(GOLDEN, 'local.expected.jsonl')) as f:
        exp = [json.loads(x) for x in f if x.strip()]
    checked = pending_docs = 0
    for log in ('local_rounds', 'local_lag'):
        src = OpBatch.load(os.path.join(GOLDEN, log + '.mtlog'))
        def pending(st):
            return any(sg[1] == -1 or (sg[3] == -1 and sg[4] != -1) for sg in st['segs'])
        # per document its last checkpoint with edits still pending, else its last one
        last = {}
        for r in exp:
            if r['log'] == log and r['states'] and not r['err']:
                pend = [c for c in r['states'] if pending(c[1])]
                last[r['doc']] = pend[-1] if pend else r['states'][-1]
        docs = sorted(last)
        # each document's records up to its last checkpoint: the engine ends in that state
        idx = np.concatenate([np.arange(int(src.row_ptr[d]), int(src.row_ptr[d]) + last[d][0]) for d in docs])
        rp = np.concatenate([[0], np.cumsum([last[d][0] for d in docs])]).astype(np.uint32)
        batch = OpBatch(src.ops[idx].copy(), src.payload, rp)
        eng = MergeEngine(len(docs), ops_per_launch=32)
        eng.apply(batch)
        rows, want = [], []
        for k, d in enumerate(docs):
            st = last[d][1]
            assert eng.state(k) == st, (log, d)
            n = sum(_view_len(s, None, 0) for s in st['segs'])
            for p in range(0, n + 2, max(1, n // 16)):
                rows.append((k, p, POS_LOCAL, 0, POS_CONTAINING))
                want.append(_expected(st, p, None, 0))
            # remote clients' views (resolveRemoteClientPosition): pending local inserts and removals
            # carry seq / removedSeq -1 (UnassignedSequenceNumber), which no refSeq has seen
            ops = src.ops[int(src.row_ptr[d]):int(src.row_ptr[d]) + last[d][0]]
            own = set(int(c) for c in ops['client'][ops['seq'] == -1])
            pending_docs += pending(st)
            clients = sorted({sg[2] for sg in st['segs'] if sg[2] > 0} - own)[:2]
            for c in clients:
                for rs in (st['msn'], st['seq']):
                    vlen = sum(_view_len(sg, rs, c) for sg in st['segs'])
                    for p in range(0, vlen + 2, max(1, vlen // 8)):
                        rows.append((k, p, rs, c, POS_CONTAINING))
                        want.append(_expected(st, p, rs, c))
        got = eng.resolve_positions(np.array(rows, dtype=POS_QUERY_DTYPE))
        for k, (g, w) in enumerate(zip(got, want)):
            if w[0] < 0:
                assert int(g['ordinal']) == -1, (log, rows[k])
            else:
                assert (int(g['ordinal']), int(g['offset']), int(g['position']), int(g['length'])) == w, (log, rows[k])
        checked += len(rows)
    assert checked > 100 and pending_docs > 0


def test_device_queries_out_of_range_are_flagged():
    """mt_resolve_positions_device takes device-resident queries the host never sees: a query naming a
    document past n_docs or an unknown kind gets ordinal MT_POS_BAD_QUERY (-2), never a read out of
    bounds, and the queries around it are answered."""
    from fluidframework_amd.engine import POS_CONTAINING, POS_LOCAL, POS_QUERY_DTYPE, POS_RESULT_DTYPE, MergeEngine
    from fluidframework_amd.hipmem import DeviceBuffer
    batch, exp = load_golden('synth_c3')
    eng = MergeEngine(batch.n_docs, ops_per_launch=32)
    eng.apply(batch)
    rows = [(0, 0, POS_LOCAL, 0, POS_CONTAINING), (batch.n_docs, 0, POS_LOCAL, 0, POS_CONTAINING),
            (1 << 30, 5, 3, 1, POS_CONTAINING), (1, 0, POS_LOCAL, 0, 7), (1, 1, POS_LOCAL, 0, POS_CONTAINING)]
    q = np.array(rows, dtype=POS_QUERY_DTYPE)
    want = eng.resolve_positions(q[[0, 4]])
    dq, dr = DeviceBuffer(q.nbytes).upload(q), DeviceBuffer(len(q) * POS_RESULT_DTYPE.itemsize)
    eng.resolve_positions_device(dq.ptr, len(q), dr.ptr)
    got = dr.download(POS_RESULT_DTYPE)
    assert list(got['ordinal'][[1, 2, 3]]) == [-2, -2, -2]
    assert got[0] == want[0] and got[4] == want[1]
