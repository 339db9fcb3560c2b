"""The contract of mt_marker_positions / mt_marker_positions_device (include/mtgpu.h "marker ids"), as
the other batched queries keep it (tests/test_query_contract.py): n == 0 writes nothing, a bad argument
is refused (MT_ERR_ARG) before anything is written, a batch answers what its queries answer one at a
time, and a device-resident query the host could not check is flagged and reads nothing."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MT_OK, MT_ERR_ARG = 0, 1
SENT = 0xA5


@pytest.fixture(scope='module')
def eng():
    from fluidframework_amd.engine import MergeEngine
    from fluidframework_amd.oplog import F_MARKER, INSERT, build_batch
    docs = [[(i + 1, i, 0, 1 + i % 2, INSERT, i, 0, '\x01' if i % 5 == 2 else 'ab', {2: 1 + i} if i % 5 == 2 else None,
              F_MARKER if i % 5 == 2 else 0) for i in range(40 + 30 * d)] for d in range(3)]
    e = MergeEngine(3, ops_per_launch=32)
    e.apply(build_batch(docs))
    yield e
    e.close()


def ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def queries(rows):
    from fluidframework_amd.engine import MARKER_QUERY_DTYPE, POS_LOCAL
    return np.array([(d, POS_LOCAL, 0, key, 0, value, 0) for d, key, value in rows], dtype=MARKER_QUERY_DTYPE)


def test_refusals_write_nothing(eng):
    from fluidframework_amd.engine import MARKER_RESULT_DTYPE, lib
    L = lib()
    out = np.full(4 * MARKER_RESULT_DTYPE.itemsize, SENT, np.uint8)
    good = queries([(0, 2, 3), (1, 2, 8)])
    for q in (queries([(0, 2, 3), (3, 2, 3)]),       # a document past the engine's
              queries([(0, 32, 3), (1, 2, 3)]),      # a key past the wide form's
              queries([(1 << 31, 2, 3)])):
        assert L.mt_marker_positions(eng.h, ptr(q), len(q), ptr(out)) == MT_ERR_ARG
        assert (out == SENT).all()
    assert L.mt_marker_positions(eng.h, None, 2, ptr(out)) == MT_ERR_ARG
    assert L.mt_marker_positions(eng.h, ptr(good), 2, None) == MT_ERR_ARG
    assert L.mt_marker_positions(None, ptr(good), 2, ptr(out)) == MT_ERR_ARG
    assert L.mt_marker_positions_device(eng.h, None, 2, 1) == MT_ERR_ARG
    assert L.mt_marker_positions_device(eng.h, 1, 2, None) == MT_ERR_ARG
    assert (out == SENT).all()


def test_n_zero_is_ok_and_writes_nothing(eng):
    from fluidframework_amd.engine import MARKER_RESULT_DTYPE, lib
    L = lib()
    out = np.full(2 * MARKER_RESULT_DTYPE.itemsize, SENT, np.uint8)
    assert L.mt_marker_positions(eng.h, None, 0, None) == MT_OK
    assert L.mt_marker_positions(eng.h, ptr(queries([(9, 40, 1)])), 0, ptr(out)) == MT_OK
    assert L.mt_marker_positions_device(eng.h, None, 0, None) == MT_OK
    assert (out == SENT).all()


@pytest.mark.parametrize('n', [1, 3, 5])
def test_batch_equals_one_at_a_time(eng, n):
    rows = [(0, 2, 3), (1, 2, 8), (2, 2, 98), (2, 2, 4), (1, 2, 0)][:n]
    got = eng.marker_positions(queries(rows))
    for i, r in enumerate(rows):
        assert got[i] == eng.marker_positions(queries([r]))[0], r
    # and they are the rule's answers on the documents' canonical states (ids 3, 8 and 98 exist)
    from fluidframework_amd.relpos import choose_marker, marker_position
    for g, (d, key, value) in zip(got, rows):
        st = eng.state(d)
        k = choose_marker(st, key, value)
        assert (k is not None) == (value in (3, 8, 98))
        assert (int(g['ordinal']), int(g['position'])) == ((-1, 0) if k is None else (k, marker_position(st, k)))


def test_device_form_flags_a_bad_query(eng):
    """A document past the engine's, or a key past 31, in device-resident queries: ordinal
    MT_POS_BAD_QUERY (-2), nothing read, and the queries around it answered."""
    from fluidframework_amd.engine import MARKER_RESULT_DTYPE
    from fluidframework_amd.hipmem import DeviceBuffer
    q = queries([(0, 2, 3), (3, 2, 3), (1 << 30, 2, 3), (1, 200, 8), (1, 2, 8)])
    want = eng.marker_positions(q[[0, 4]])
    dq, dr = DeviceBuffer(q.nbytes).upload(q), DeviceBuffer(len(q) * MARKER_RESULT_DTYPE.itemsize)
    eng.marker_positions_device(dq.ptr, len(q), dr.ptr)
    got = dr.download(MARKER_RESULT_DTYPE)
    assert list(got['ordinal'][[1, 2, 3]]) == [-2, -2, -2]
    assert got[0] == want[0] and got[4] == want[1]
