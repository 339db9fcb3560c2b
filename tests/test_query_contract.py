"""The contract of the batched query entries of include/mtgpu.h, as the host wrappers keep it
(csrc/mt_queries.cpp): what a call writes for n == 0, that a query naming a document that does not
exist is refused (MT_ERR_ARG) before anything is written, and that a batch of n = 1, 3 and 5 queries
answers, element by element, what the same queries answer one at a time -- odd counts of the 12-byte
and 4-byte records are where a mis-carved scratch buffer shows.  The two two-pass readers' sizing,
too-small and exact calls, the fold that the add / remove calls run even for n == 0, and the event
drain's sizing / draining / sizing sequence.

One engine of 3 documents with the first 200 records per document of synth_c3 (as
test_intervals.test_lifecycle), events, 8 references and 2 intervals per document.  The C entries are
called through ctypes where the Python methods hide the case (n == 0, a too-small capacity)."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

N_DOCS = 3
EVCAP = 1 << 12
MT_OK, MT_ERR_ARG = 0, 1
SENT = 0xA5
SEG_INFO_BYTES = 168


def cut(batch, lo, hi):
    from fluidframework_amd.oplog import OpBatch
    idx, rp = [], [0]
    for d in range(N_DOCS):
        base = int(batch.row_ptr[d])
        idx.append(np.arange(base + lo, base + hi))
        rp.append(rp[-1] + hi - lo)
    return OpBatch(batch.ops[np.concatenate(idx).astype(np.int64)].copy(), batch.payload, np.array(rp, dtype=np.uint32))


@pytest.fixture(scope='module')
def log():
    from fluidframework_amd.oplog import OpBatch
    return OpBatch.load(os.path.join(GOLDEN, 'synth_c3.mtlog'))


def make_engine(log, intervals=((0, 2, 6),)):
    """The set-up engine: two references per document (handles 0 and 1), and the given intervals
    (document, start, end), one call each so that their handles are determined."""
    from fluidframework_amd.engine import MergeEngine
    eng = MergeEngine(N_DOCS, ops_per_launch=32).enable_events(EVCAP).enable_refs(8).enable_intervals(2)
    eng.apply(cut(log, 0, 200))
    assert all(eng.length(d) > 12 for d in range(N_DOCS))
    assert eng.add_refs([0, 1, 2], [1, 2, 3], [0, 0, 0]).tolist() == [0, 0, 0]
    assert eng.add_refs([0, 1, 2], [5, 6, 7], [0, 0, 0]).tolist() == [1, 1, 1]
    for d, a, b in intervals:
        assert int(eng.add_intervals([d], [a], [b], [0])[0]) < 2
    return eng


@pytest.fixture(scope='module')
def eng(log):
    """shared by the tests that only read: five intervals over the three documents"""
    e = make_engine(log, ((0, 2, 6), (0, 4, 9), (1, 1, 4), (1, 3, 11), (2, 0, 5)))
    yield e
    e.close()


def L():
    from fluidframework_amd.engine import lib
    L_ = lib()
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    L_.mt_segment_infos.argtypes = [vp, vp, vp, u32, vp]
    L_.mt_segment_infos.restype = ctypes.c_int
    return L_


def ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def sent(n, dtype=np.uint8):
    """n records of `dtype`, every byte the sentinel"""
    return np.frombuffer(bytes([SENT]) * (np.dtype(dtype).itemsize * n), dtype=dtype).copy()


def untouched(*arrays):
    return all((a.view(np.uint8) == SENT).all() for a in arrays)


# ---- the queries, five of each, documents 0 1 2 0 1 --------------------------------------------
def docs5():
    return np.array([0, 1, 2, 0, 1], dtype=np.uint32)


def tile_q():
    from fluidframework_amd.engine import TILE_QUERY_DTYPE
    q = np.zeros(5, dtype=TILE_QUERY_DTYPE)
    q['doc'], q['pos'], q['preceding'] = docs5(), [1, 4, 7, 10, 12], [0, 1, 0, 1, 0]
    q['vmask'] = 0xFFFFFFFF
    return q


def pos_q():
    from fluidframework_amd.engine import POS_LOCAL, POS_QUERY_DTYPE
    q = np.zeros(5, dtype=POS_QUERY_DTYPE)
    q['doc'], q['pos'], q['ref_seq'] = docs5(), [0, 3, 6, 9, 12], POS_LOCAL
    return q


def iv_q():
    from fluidframework_amd.intervals import INTERVAL_QUERY_DTYPE
    q = np.zeros(5, dtype=INTERVAL_QUERY_DTYPE)
    q['doc'], q['start'], q['end'] = docs5(), [0, 0, 0, 3, 2], [12, 12, 12, 5, 3]
    return q


def text_q():
    from fluidframework_amd.engine import MergeEngine
    from fluidframework_amd.textread import TEXT_MARKERS
    return MergeEngine.text_queries(docs5(), starts=[0, 1, 2, 3, 4], ends=[12, 9, 11, 4, 12], placeholders='*',
                                    flags=TEXT_MARKERS)


class Call:
    """One batched read: run(eng, lo, hi) sends queries [lo, hi) and returns (status, the outputs as a
    list of arrays, one row per query); the outputs are filled with the sentinel before the call."""

    def __init__(self, name, run):
        self.name, self.run = name, run


def _tiles(eng, lo, hi, q=None):
    from fluidframework_amd.engine import TILE_RESULT_DTYPE
    q = tile_q()[lo:hi] if q is None else q
    out = sent(len(q), TILE_RESULT_DTYPE)
    return L().mt_find_tiles(eng.h, ptr(q), len(q), ptr(out)), [out]


def _resolve(eng, lo, hi, q=None):
    from fluidframework_amd.engine import POS_RESULT_DTYPE
    q = pos_q()[lo:hi] if q is None else q
    out = sent(len(q), POS_RESULT_DTYPE)
    return L().mt_resolve_positions(eng.h, ptr(q), len(q), ptr(out)), [out]


def _seginfos(eng, lo, hi, docs=None):
    docs = docs5()[lo:hi] if docs is None else docs
    ords = np.array([0, 1, 2, 3, 1], dtype=np.int32)[lo:lo + len(docs)]
    out = sent(len(docs) * SEG_INFO_BYTES).reshape(len(docs), SEG_INFO_BYTES)
    return L().mt_segment_infos(eng.h, ptr(docs), ptr(ords), len(docs), ptr(out)), [out]


def _stacks(eng, lo, hi, q=None):
    from fluidframework_amd.engine import STACK_ITEM_DTYPE
    q = tile_q()[lo:hi] if q is None else q
    cap = 3  # (an odd number of 12-byte items per query)
    items, depth = sent(len(q) * cap, STACK_ITEM_DTYPE).reshape(len(q), cap), sent(len(q), np.uint32)
    st = L().mt_range_stacks(eng.h, ptr(q), len(q), cap, ptr(items), ptr(depth))
    if st == MT_OK:  # (the items above a stack's depth are whatever the scratch held: not part of the answer)
        for i in range(len(q)):
            items[i, min(cap, int(depth[i]) & 0x7FFFFFFF):] = 0
    return st, [items, depth]


def _ref_positions(eng, lo, hi, docs=None):
    from fluidframework_amd.refs import REF_POS_DTYPE
    docs = docs5()[lo:hi] if docs is None else docs
    h = np.array([0, 1, 0, 1, 0], dtype=np.uint32)[lo:lo + len(docs)]
    out = sent(len(docs), REF_POS_DTYPE)
    return L().mt_refs_positions(eng.h, ptr(docs), ptr(h), len(docs), ptr(out)), [out]


def _iv_positions(eng, lo, hi, docs=None):
    from fluidframework_amd.intervals import INTERVAL_POS_DTYPE
    docs = docs5()[lo:hi] if docs is None else docs
    out = sent(len(docs) * 2, INTERVAL_POS_DTYPE).reshape(len(docs), 2)
    return L().mt_intervals_positions(eng.h, ptr(docs), len(docs), ptr(out)), [out]


def _text_lengths(eng, lo, hi, q=None):
    from fluidframework_amd.textread import TEXT_COUNT_DTYPE
    q = text_q()[lo:hi] if q is None else q
    out = sent(len(q), TEXT_COUNT_DTYPE)
    return L().mt_text_lengths(eng.h, ptr(q), len(q), ptr(out)), [out]


FLAT = [Call('mt_find_tiles', _tiles), Call('mt_resolve_positions', _resolve), Call('mt_segment_infos', _seginfos),
        Call('mt_range_stacks', _stacks), Call('mt_refs_positions', _ref_positions),
        Call('mt_intervals_positions', _iv_positions), Call('mt_text_lengths', _text_lengths)]


def overlapping(eng, q, cap=None, sizing=False):
    """(status, row_ptr, out, total) of mt_intervals_overlapping; cap None: the sizing call's total"""
    rp, total = sent(len(q) + 1, np.uint32), ctypes.c_uint64(0x5A5A5A5A)
    if sizing:
        return L().mt_intervals_overlapping(eng.h, ptr(q), len(q), ptr(rp), None, 0, ctypes.byref(total)), rp, None, total.value
    if cap is None:
        st, rp0, _, cap = overlapping(eng, q, sizing=True)
        assert st == MT_OK
    out = sent(max(1, cap), np.uint32)
    st = L().mt_intervals_overlapping(eng.h, ptr(q), len(q), ptr(rp), ptr(out), cap, ctypes.byref(total))
    return st, rp, out, total.value


def text_ranges(eng, q, cap=None, m_cap=None, sizing=False):
    """(status, row_ptr, units, m_row_ptr, markers, totals) of mt_text_ranges"""
    from fluidframework_amd.textread import TEXT_MARKER_DTYPE
    rp, mrp, totals = sent(len(q) + 1, np.uint32), sent(len(q) + 1, np.uint32), sent(2, np.uint64)
    if sizing:
        st = L().mt_text_ranges(eng.h, ptr(q), len(q), ptr(rp), None, 0, ptr(mrp), None, 0, ptr(totals))
        return st, rp, None, mrp, None, totals
    if cap is None:
        st, _, _, _, _, t = text_ranges(eng, q, sizing=True)
        assert st == MT_OK
        cap, m_cap = int(t[0]), int(t[1])
    units, marks = sent(max(1, cap), np.uint16), sent(max(1, m_cap), TEXT_MARKER_DTYPE)
    st = L().mt_text_ranges(eng.h, ptr(q), len(q), ptr(rp), ptr(units), cap, ptr(mrp), ptr(marks), m_cap, ptr(totals))
    return st, rp, units, mrp, marks, totals


# ---- n == 0 -----------------------------------------------------------------------------------
@pytest.mark.parametrize('call', FLAT, ids=lambda c: c.name)
def test_no_queries_write_nothing(eng, call):
    st, outs = call.run(eng, 0, 0)
    assert st == MT_OK and untouched(*outs)


def test_no_queries_two_pass(eng):
    """row_ptr[0] == 0 and totals 0; nothing else touched"""
    st, rp, out, total = overlapping(eng, iv_q()[:0], cap=4)
    assert st == MT_OK and rp.tolist() == [0] and total == 0 and untouched(out)
    st, rp, units, mrp, marks, totals = text_ranges(eng, text_q()[:0], cap=4, m_cap=4)
    assert st == MT_OK and rp.tolist() == [0] and mrp.tolist() == [0] and totals.tolist() == [0, 0]
    assert untouched(units, marks)


def test_no_adds_or_removes(eng):
    h = sent(1, np.uint32)
    for fn in (L().mt_refs_add, L().mt_intervals_add, L().mt_intervals_remove):
        assert fn(eng.h, None, 0, ptr(h)) == MT_OK and untouched(h)
    assert L().mt_refs_remove(eng.h, None, None, 0) == MT_OK


# ---- a query of a document that does not exist --------------------------------------------------
def bad_docs():
    return np.array([0, N_DOCS, 1], dtype=np.uint32)


def with_bad_doc(q):
    q = q[:3].copy()
    q['doc'] = bad_docs()
    return q


def test_unknown_document_is_refused_before_anything_is_written(eng):
    runs = [_tiles(eng, 0, 3, with_bad_doc(tile_q())), _resolve(eng, 0, 3, with_bad_doc(pos_q())),
            _seginfos(eng, 0, 3, bad_docs()), _stacks(eng, 0, 3, with_bad_doc(tile_q())),
            _ref_positions(eng, 0, 3, bad_docs()), _iv_positions(eng, 0, 3, bad_docs()),
            _text_lengths(eng, 0, 3, with_bad_doc(text_q()))]
    for (st, outs), call in zip(runs, FLAT):
        assert st == MT_ERR_ARG and untouched(*outs), call.name
    st, rp, out, total = overlapping(eng, with_bad_doc(iv_q()), cap=8)
    assert st == MT_ERR_ARG and untouched(rp, out) and total == 0x5A5A5A5A
    st, rp, units, mrp, marks, totals = text_ranges(eng, with_bad_doc(text_q()), cap=64, m_cap=8)
    assert st == MT_ERR_ARG and untouched(rp, units, mrp, marks, totals)


def test_unknown_document_is_refused_by_adds_and_removes(eng):
    from fluidframework_amd.intervals import INTERVAL_ADD_DTYPE
    from fluidframework_amd.refs import REF_ADD_DTYPE
    before = _ref_positions(eng, 0, 5)[1][0], _iv_positions(eng, 0, 3)[1][0]
    h = sent(3, np.uint32)
    a = np.zeros(3, dtype=REF_ADD_DTYPE)
    a['doc'], a['pos'] = bad_docs(), 1
    assert L().mt_refs_add(eng.h, ptr(a), 3, ptr(h)) == MT_ERR_ARG and untouched(h)
    assert L().mt_refs_remove(eng.h, ptr(bad_docs()), ptr(np.zeros(3, dtype=np.uint32)), 3) == MT_ERR_ARG
    ia = np.zeros(3, dtype=INTERVAL_ADD_DTYPE)
    ia['doc'], ia['start'], ia['end'] = bad_docs(), 1, 2
    assert L().mt_intervals_add(eng.h, ptr(ia), 3, ptr(h)) == MT_ERR_ARG and untouched(h)
    q = with_bad_doc(iv_q())
    q['start'], q['end'] = [2, 2, 1], [6, 6, 4]  # (intervals that exist: none may go)
    assert L().mt_intervals_remove(eng.h, ptr(q), 3, ptr(h)) == MT_ERR_ARG and untouched(h)
    after = _ref_positions(eng, 0, 5)[1][0], _iv_positions(eng, 0, 3)[1][0]
    assert all(np.array_equal(x, y) for x, y in zip(before, after))


# ---- a batch answers what its queries answer one at a time ------------------------------------
@pytest.fixture(scope='module')
def singles(eng):
    """every flat call's answers to its five queries, one query per call"""
    out = {}
    for call in FLAT:
        rows = [call.run(eng, i, i + 1) for i in range(5)]
        assert all(st == MT_OK for st, _ in rows), call.name
        out[call.name] = [np.concatenate([r[1][k] for r in rows]) for k in range(len(rows[0][1]))]
    return out


@pytest.mark.parametrize('n', [1, 3, 5])
@pytest.mark.parametrize('call', FLAT, ids=lambda c: c.name)
def test_batch_equals_one_at_a_time(eng, singles, call, n):
    st, outs = call.run(eng, 0, n)
    assert st == MT_OK
    assert not all(untouched(o) for o in outs)
    for got, one in zip(outs, singles[call.name]):
        assert np.array_equal(got, one[:n]), (call.name, n)


def test_the_answers_are_not_trivial(eng, singles):
    """the batches above compare answers that say something: references and intervals with positions,
    segments that exist, text of the asked lengths"""
    assert (singles['mt_refs_positions'][0]['position'] >= 0).all()
    assert int(singles['mt_intervals_positions'][0]['live'].sum()) == 9  # (documents 0 1 2 0 1: 2 + 2 + 1 + 2 + 2)
    assert (singles['mt_resolve_positions'][0]['ordinal'] >= 0).all()
    assert singles['mt_text_lengths'][0]['units'].tolist() == [12, 8, 9, 1, 8]
    assert (singles['mt_segment_infos'][0].view('<i4')[:, 0] != -2**31).all()  # (seq: the segments exist)


@pytest.mark.parametrize('n', [1, 3, 5])
def test_two_pass_batch_equals_one_at_a_time(eng, n):
    q = iv_q()
    st, rp, out, total = overlapping(eng, q[:n])
    assert st == MT_OK and rp[0] == 0 and rp[n] == total
    rows = [overlapping(eng, q[i:i + 1]) for i in range(n)]
    assert [out[rp[i]:rp[i + 1]].tolist() for i in range(n)] == [r[2][:r[3]].tolist() for r in rows]
    if n == 5:
        assert total >= 5  # (each of the first three queries covers its document's intervals)
    tq = text_q()
    st, rp, units, mrp, marks, totals = text_ranges(eng, tq[:n])
    assert st == MT_OK and rp[0] == 0 and mrp[0] == 0 and totals.tolist() == [rp[n], mrp[n]]
    rows = [text_ranges(eng, tq[i:i + 1]) for i in range(n)]
    assert [units[rp[i]:rp[i + 1]].tolist() for i in range(n)] == [r[2][:int(r[5][0])].tolist() for r in rows]
    assert [marks[mrp[i]:mrp[i + 1]].tolist() for i in range(n)] == [r[4][:int(r[5][1])].tolist() for r in rows]
    assert [int(rp[i + 1] - rp[i]) for i in range(n)] == [12, 8, 9, 1, 8][:n]


def test_two_pass_capacities(eng):
    """a sizing call fills the rows and totals; a capacity one short is refused with the same rows and
    totals, the exact capacity answers"""
    q = iv_q()
    st, rp0, _, total0 = overlapping(eng, q, sizing=True)
    assert st == MT_OK and total0 >= 5 and rp0[0] == 0 and rp0[5] == total0
    st, rp, out, total = overlapping(eng, q, cap=total0 - 1)
    assert st == MT_ERR_ARG and rp.tolist() == rp0.tolist() and total == total0 and untouched(out)
    st, rp, out, total = overlapping(eng, q, cap=total0)
    assert st == MT_OK and rp.tolist() == rp0.tolist() and total == total0 and not untouched(out[:total0])
    tq = text_q()
    st, rp0, _, mrp0, _, t0 = text_ranges(eng, tq, sizing=True)
    assert st == MT_OK and t0.tolist() == [38, mrp0[5]] and rp0.tolist() == [0, 12, 20, 29, 30, 38]
    short = [(int(t0[0]) - 1, int(t0[1]))] + ([(int(t0[0]), int(t0[1]) - 1)] if t0[1] else [])
    for cap, m_cap in short:
        st, rp, units, mrp, marks, t = text_ranges(eng, tq, cap=cap, m_cap=m_cap)
        assert st == MT_ERR_ARG and rp.tolist() == rp0.tolist() and mrp.tolist() == mrp0.tolist()
        assert t.tolist() == t0.tolist() and untouched(units, marks)
    st, rp, units, mrp, marks, t = text_ranges(eng, tq, cap=int(t0[0]), m_cap=int(t0[1]))
    assert st == MT_OK and rp.tolist() == rp0.tolist() and t.tolist() == t0.tolist() and (units[:38] != 0xA5A5).all()


# ---- adds and removes: batches on one engine, one at a time on another ---------------------------
def by_doc(docs, handles):
    return {d: sorted(int(h) for dd, h in zip(docs, handles) if dd == d) for d in set(docs)}


@pytest.mark.parametrize('n', [1, 3, 5])
def test_refs_add_and_remove_batches(log, n):
    """Entries of one document claim their slots concurrently, so which entry gets which of the
    document's free handles is not determined: the handles are compared per document as sets, and
    element by element through the position each handle then answers."""
    a, b = make_engine(log), make_engine(log)
    docs, pos = [0, 1, 1, 2, 2][:n], [9, 10, 11, 8, 12][:n]
    ha = a.add_refs(docs, pos, [0] * n)
    hb = np.concatenate([b.add_refs(docs[i:i + 1], pos[i:i + 1], [0]) for i in range(n)])
    assert by_doc(docs, ha) == by_doc(docs, hb) and all(h in (2, 3, 4) for h in ha.tolist())
    pa, pb = a.ref_positions(docs, ha), b.ref_positions(docs, hb)
    assert np.array_equal(pa, pb) and pa['position'].tolist() == pos
    # remove them as one batch / one at a time: the same references are left
    a.remove_refs(docs, ha)
    for i in range(n):
        b.remove_refs(docs[i:i + 1], hb[i:i + 1])
    every = [(d, h) for d in range(N_DOCS) for h in range(8)]
    ed, eh = [d for d, _ in every], [h for _, h in every]
    left = a.ref_positions(ed, eh)
    assert np.array_equal(left, b.ref_positions(ed, eh))
    gone = set(zip(docs, ha.tolist()))
    for (d, h), p in zip(every, left):
        if (d, h) in gone:
            assert p['ordinal'] == -2, (d, h)  # (no such reference)
        elif h < 2:
            assert p['position'] >= 0, (d, h)  # (the set-up's references stay)
    a.close()
    b.close()


@pytest.mark.parametrize('n', [1, 3, 5])
def test_intervals_add_and_remove_batches(log, n):
    a, b = make_engine(log), make_engine(log)
    docs, s, t = [0, 1, 1, 2, 2][:n], [1, 2, 3, 4, 5][:n], [8, 9, 10, 11, 12][:n]
    ha = a.add_intervals(docs, s, t, [0] * n)
    hb = np.concatenate([b.add_intervals(docs[i:i + 1], s[i:i + 1], t[i:i + 1], [0]) for i in range(n)])
    assert by_doc(docs, ha) == by_doc(docs, hb) and all(h < 2 for h in ha.tolist())
    pa, pb = a.interval_positions(range(N_DOCS)), b.interval_positions(range(N_DOCS))
    ends = lambda p, d, h: (int(p[d][h]['start']), int(p[d][h]['end']), int(p[d][h]['live']))  # noqa: E731
    assert [ends(pa, d, h) for d, h in zip(docs, ha)] == [ends(pb, d, h) for d, h in zip(docs, hb)] == \
        [(x, y, 1) for x, y in zip(s, t)]
    ra = a.remove_intervals(docs, s, t)
    rb = np.concatenate([b.remove_intervals(docs[i:i + 1], s[i:i + 1], t[i:i + 1]) for i in range(n)])
    assert ra.tolist() == ha.tolist() and rb.tolist() == hb.tolist()
    pa, pb = a.interval_positions(range(N_DOCS)), b.interval_positions(range(N_DOCS))
    assert pa['live'].tolist() == pb['live'].tolist() == [[1, 0], [0, 0], [0, 0]]
    a.close()
    b.close()


# ---- the fold runs for n == 0 -------------------------------------------------------------------
def test_empty_adds_and_removes_still_fold(log):
    """With undrained events an add or remove of nothing still moves the references; the positions
    asked next are those of an engine that drained (and so folded) first."""
    every = [(d, h) for d in range(N_DOCS) for h in range(4)]
    ed, eh = [d for d, _ in every], [h for _, h in every]
    base = make_engine(log)
    base.drain_events()
    before = base.ref_positions(ed, eh)
    base.apply(cut(log, 200, 400))
    base.drain_events()
    want = base.ref_positions(ed, eh)
    assert not np.array_equal(before, want)  # (the second 200 records moved some reference)
    base.close()
    h = sent(1, np.uint32)
    calls = {'mt_refs_add': lambda e: L().mt_refs_add(e.h, None, 0, ptr(h)),
             'mt_refs_remove': lambda e: L().mt_refs_remove(e.h, None, None, 0),
             'mt_intervals_add': lambda e: L().mt_intervals_add(e.h, None, 0, ptr(h)),
             'mt_intervals_remove': lambda e: L().mt_intervals_remove(e.h, None, 0, ptr(h))}
    for name, fn in calls.items():
        e = make_engine(log)
        e.drain_events()
        e.apply(cut(log, 200, 400))
        assert fn(e) == MT_OK and untouched(h), name
        assert np.array_equal(e.ref_positions(ed, eh), want), name
        e.close()


# ---- the event drain ----------------------------------------------------------------------------
def test_events_drain_sizing_draining_sizing(log):
    from fluidframework_amd.events import EVENT_DTYPE
    e = make_engine(log)
    rp0, total = sent(N_DOCS + 1, np.uint32), ctypes.c_uint64(0)
    assert L().mt_events_drain(e.h, None, 0, ptr(rp0), ctypes.byref(total)) == MT_OK
    n = total.value
    assert n > 0 and rp0[0] == 0 and rp0[N_DOCS] == n and (np.diff(rp0.astype(np.int64)) > 0).all()
    rows, rp = sent(n, EVENT_DTYPE), sent(N_DOCS + 1, np.uint32)
    assert L().mt_events_drain(e.h, ptr(rows), n - 1, ptr(rp), ctypes.byref(total)) == MT_ERR_ARG  # nothing cleared
    assert rp.tolist() == rp0.tolist() and total.value == n and untouched(rows)
    assert L().mt_events_drain(e.h, ptr(rows), n, ptr(rp), ctypes.byref(total)) == MT_OK
    assert rp.tolist() == rp0.tolist() and total.value == n
    assert not any(untouched(rows[rp[d]:rp[d] + 1]) for d in range(N_DOCS))
    assert L().mt_events_drain(e.h, None, 0, ptr(rp), ctypes.byref(total)) == MT_OK
    assert rp.tolist() == [0] * (N_DOCS + 1) and total.value == 0
    e.close()
