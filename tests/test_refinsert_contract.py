"""The contract of mt_refs_insert_local (include/mtgpu.h "local references", csrc/mt_queries.cpp), through
ctypes: every refusal is MT_ERR_ARG before any device work -- nothing written, nothing applied -- for
references not enabled, NULL pointers with n > 0, unknown documents, two inserts of one document,
documents out of order, a record of another kind and a payload out of bounds; n == 0 succeeds and
launches nothing; a detached reference and a handle that names none answer -1 / MT_REF_BAD_HANDLE and
leave the checksum and the event buffer as they were, beside a record of the same call that applies."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MT_OK, MT_ERR_ARG = 0, 1
SENT = 0x5A5A5A5A
N_DOCS = 4


def ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def make_engine(refs=True):
    """Four documents 'abcdef' + 'gh' with c1's pending removal of 'b'; references: handle 0 on 'cdef'
    offset 1 everywhere, handle 1 on 'gh' (document 2's is detached by a remote removal)."""
    from fluidframework_amd.engine import MergeEngine
    from fluidframework_amd.oplog import INSERT, REMOVE, build_batch
    base = [(1, 0, 0, 2, INSERT, 0, 0, 'abcdef', None, 0), (2, 1, 0, 3, INSERT, 6, 0, 'gh', None, 0),
            (-1, 0, 0, 1, REMOVE, 1, 2, None, None, 0)]
    eng = MergeEngine(N_DOCS, ops_per_launch=8).enable_events(256)
    eng.apply(build_batch([base] * N_DOCS))
    if refs:
        eng.enable_refs(4)
        assert eng.add_refs(range(N_DOCS), [2] * N_DOCS, [0] * N_DOCS).tolist() == [0] * N_DOCS
        assert eng.add_refs(range(N_DOCS), [5] * N_DOCS, [0] * N_DOCS).tolist() == [1] * N_DOCS
        eng.apply(build_batch([[], [], [(3, 2, 0, 2, REMOVE, 6, 8, None, None, 0)], []]))
    return eng


def records(n, text=b'XY'):
    from fluidframework_amd.oplog import OP_DTYPE
    ops = np.zeros(n, dtype=OP_DTYPE)
    ops['seq'], ops['client'] = -1, 1
    ops['payload_off'] = len(text) * np.arange(n)
    ops['payload_len'] = len(text)
    return ops, np.frombuffer(text * max(n, 1), dtype=np.uint8).copy()


def at(*pairs):
    from fluidframework_amd.refs import REF_INSERT_DTYPE
    return np.array(list(pairs), dtype=REF_INSERT_DTYPE)


def call(eng, a, ops, n, pay, nbytes, out):
    from fluidframework_amd.engine import lib
    return lib().mt_refs_insert_local(eng.h if eng is not None else None, ptr(a), ptr(ops), n, ptr(pay), nbytes, ptr(out))


def test_refusals_apply_nothing():
    eng = make_engine()
    eng.drain_events()
    before = eng.checksums().tolist()
    ops, pay = records(2)
    out = np.full(2, SENT, dtype=np.int32)
    good = at((0, 0), (1, 0))
    seqd, removal, lowered = ops.copy(), ops.copy(), ops.copy()
    seqd['seq'][1] = 5
    removal['type'][1] = 1
    lowered['type'][0] = 5
    far = ops.copy()
    far['payload_off'][1] = len(pay) - 1
    cases = [(None, ops, pay, out), (good, None, pay, out), (good, ops, pay, None), (good, ops, None, out),
             (at((0, 0), (N_DOCS, 0)), ops, pay, out),   # a document past the engine's
             (at((1, 0), (1, 1)), ops, pay, out),        # two inserts of one document
             (at((2, 0), (1, 0)), ops, pay, out),        # documents out of order
             (good, seqd, pay, out), (good, removal, pay, out), (good, lowered, pay, out), (good, far, pay, out)]
    for i, (a, o, p, res) in enumerate(cases):
        assert call(eng, a, o, 2, p, len(pay), res) == MT_ERR_ARG, i
    assert call(eng, good, ops, 2, pay, len(pay) - 1, out) == MT_ERR_ARG   # the last payload ends past the bytes
    assert call(None, good, ops, 2, pay, len(pay), out) == MT_ERR_ARG
    assert out.tolist() == [SENT, SENT]
    assert eng.checksums().tolist() == before and eng.drain_events() == [[]] * N_DOCS
    eng.close()
    plain = make_engine(refs=False)   # references not enabled
    assert call(plain, good, ops, 2, pay, len(pay), out) == MT_ERR_ARG and out.tolist() == [SENT, SENT]
    plain.close()


def test_zero_inserts_launch_nothing():
    eng = make_engine()
    eng.drain_events()
    before = eng.checksums().tolist()
    stats = eng.last_stats()
    out = np.full(1, SENT, dtype=np.int32)
    assert call(eng, None, None, 0, None, 0, None) == MT_OK
    assert call(eng, at((9, 9)), records(1)[0], 0, None, 0, out) == MT_OK and out.tolist() == [SENT]
    assert eng.last_stats() == stats
    assert eng.checksums().tolist() == before and eng.drain_events() == [[]] * N_DOCS
    eng.close()


def test_detached_and_bad_handles_leave_the_document_alone():
    from fluidframework_amd.refs import DETACHED, REF_BAD_HANDLE
    eng = make_engine()
    eng.drain_events()
    before = eng.checksums().tolist()
    state2 = eng.state(2)
    # document 0 applies; 1 names a free handle and 3 one past the table; 2's reference is detached
    pos = eng.insert_at_refs([0, 1, 2, 3], [0, 3, 1, 77], [(1, 'XY', None, 0)] * 4)
    assert pos.tolist() == [2, REF_BAD_HANDLE, DETACHED, REF_BAD_HANDLE]
    after = eng.checksums().tolist()
    assert after[1:] == before[1:] and after[0] != before[0]
    ev = eng.drain_events()
    assert ev[1:] == [[]] * 3 and [e[:2] for e in ev[0]] == [[-1, -2], [-1, 0]]
    assert [eng.error(d) for d in range(N_DOCS)] == [(0, 0)] * N_DOCS
    assert eng.state(2) == state2
    assert [s[0] for s in eng.state(0)['segs']] == ['a', 'b', 'c', 'XY', 'def', 'gh']
    # the documents go on: the next local edit of document 2 is its second pending edit, acked in order
    from fluidframework_amd.oplog import INSERT, REMOVE, build_batch
    eng.apply(build_batch([[], [], [(-1, 0, 0, 1, INSERT, 0, 0, 'Q', None, 0), (4, 2, 0, 1, REMOVE, 1, 2, None, None, 0),
                                    (5, 3, 0, 1, INSERT, 0, 0, 'Q', None, 0)], []]))
    assert eng.error(2) == (0, 0)
    assert [(s[0], s[1], s[3]) for s in eng.state(2)['segs']][:3] == [('Q', 5, -1), ('a', 1, -1), ('b', 1, 4)]
    eng.close()
