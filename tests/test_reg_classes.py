"""The inputs of test_reg_classes_gpu.py are what they claim (tests/reg_classes.py), checked on the CPU
oracle: every log replays without an error other than the ones it is about, the arena scenarios leave
the engine no right outcome but "no arena error", non-op padding moves nothing but the current sequence
number, and the launch sizes steer a document to the class they are meant to."""
import numpy as np
import pytest

import reg_classes as rc
from reg_classes import ARENA, FRESH, INSERT, K_ALL, K_HALT, NOOP, class_for, class_params, launch_size

EV_APPEND, EV_UNLINK, EV_INSERT = -1, -3, 0


def test_class_parameters_are_the_engines():
    """kClassParams of mt_engine.cpp for the 15 register classes, restated"""
    table = [128, 128, 40, 192, 192, 128, 40, 192, 256, 128, 40, 192, 320, 160, 48, 224,
             384, 192, 56, 256, 448, 224, 64, 288, 512, 256, 72, 320, 576, 288, 80, 352,
             640, 320, 88, 384, 704, 352, 96, 416, 768, 384, 104, 448, 832, 416, 112, 480,
             896, 448, 120, 512, 960, 480, 128, 544, 1024, 512, 136, 576]
    assert [v for K in K_ALL for v in class_params(K)] == table


def _boundaries(fn):
    """what class_for answers for a new document at launch_size(K) and one record less, K = 5 ... 16"""
    return [(fn(*FRESH, launch_size(K)), fn(*FRESH, launch_size(K) - 1)) for K in range(5, 17)]


def test_launch_size_is_the_smallest_that_reaches_its_class():
    # one record less fits the class below -- at K = 5 that is the 128 class: 128 / 192 / 256 share the
    # interior-block limit of 40 that n = 40 is the first to miss, so no launch size alone reaches K = 3, 4
    assert _boundaries(class_for) == [(K, K - 1 if K > 5 else 2) for K in range(5, 17)]
    # the three small classes at 32 records: the segment count decides
    for K, top in ((2, 62), (3, 126), (4, 190)):
        assert class_for(top, 1, 0, 0, 1, launch_size(K)) == K  # (with one empty leaf block's padding slot)
        assert class_for(top + 1, 1, 0, 0, 1, launch_size(K)) == K + 1
    # a small document stays in class K up to nseg = 48 K - 1 - n_empty (the workloads keep one below)
    for K in range(5, 17):
        n = launch_size(K)
        assert class_for(48 * K - 2 - 3, 16 * K - 1, 7, 48, 3, n) == K
        assert class_for(48 * K - 1 - 3, 16 * K - 1, 7, 48, 3, n) == K
        assert class_for(48 * K - 3, 16 * K - 1, 7, 48, 3, n) == (K + 1 if K < 16 else None)
        assert class_for(10, 16 * K, 0, 10, 0, n) == class_for(10, 5, 0, 49, 0, n) == (K + 1 if K < 16 else None)
        assert class_for(10, 5, 8, 10, 0, n) == (K + 1 if K < 16 else None)


def test_a_class_rule_off_by_one_is_noticed():
    """the check above can fail: the same rule with one `<=` turned into `<`"""
    def off_by_one(nseg, nb0, ib_need, heap_n, n_empty, n):
        for K in K_ALL:
            cap, lb, ib, h = class_params(K)
            if nseg + 2 * n + n_empty + 1 <= cap and nb0 + 2 * n + 1 <= lb and ib_need + n + 1 < ib and \
                    heap_n + 4 * n + 16 <= h:
                return K
    assert _boundaries(off_by_one) != _boundaries(class_for)


def _noop_at(o, seq, n_docs=1):
    """one non-op message per document at sequence number seq (the msn and everything else stay)"""
    from fluidframework_amd.oplog import OP_DTYPE, OpBatch
    ops = np.zeros(n_docs, dtype=OP_DTYPE)
    ops['seq'], ops['ref_seq'], ops['type'], ops['client'] = seq, seq - 1, NOOP, 1
    ops['msn'] = [o.state(d)['msn'] for d in range(n_docs)]
    return o.apply(OpBatch(ops, np.zeros(1, np.uint8), np.arange(n_docs + 1, dtype=np.uint32)))


def _same_but_seq(a, b):
    """oracle states equal in every field but `seq`, the one a non-op message moves: msn, every
    segment (text, seq, client, removal, overlap, props) and the tree's shape"""
    assert set(a) == set(b)
    return all(a[k] == b[k] for k in a if k != 'seq')


def test_pad_tail_records():
    batches = rc.scenario_batches('A2')
    p = rc.pad_tail(batches[0], 20)
    assert np.diff(p.row_ptr).tolist() == [20]
    tail = p.ops[6:]
    assert tail['seq'].tolist() == list(range(7, 21)) and tail['ref_seq'].tolist() == list(range(6, 20))
    assert set(tail['msn'].tolist()) == {5} and set(tail['client'].tolist()) == {1} and set(tail['type'].tolist()) == {NOOP}
    assert p.ops[:6].tobytes() == batches[0].ops.tobytes()
    with pytest.raises(ValueError):
        rc.pad_tail(batches[0], 5)


@pytest.mark.parametrize('name', ['A2', 'A3', 'A5'])
def test_tail_padding_moves_nothing_but_the_sequence_number(name):
    _, plain = rc.scenario(name)
    _, padded = rc.scenario(name, launch_size(9))
    assert plain.state(0)['seq'] + launch_size(9) - len(rc.SCENARIOS[name][0]) == padded.state(0)['seq']
    assert _same_but_seq(plain.state(0), padded.state(0))
    assert plain.text(0) == padded.text(0) and plain.events(0) == padded.events(0)
    # (the checksum covers the current sequence number: one non-op message at the padded log's last
    # sequence number brings the unpadded document to the same one)
    assert int(plain.checksums()[0]) != int(padded.checksums()[0])
    again = _noop_at(rc.scenario.__wrapped__(name)[1], padded.state(0)['seq'])
    assert int(again.checksums()[0]) == int(padded.checksums()[0])


def test_padding_that_moved_the_msn_is_noticed(oracle_lib):
    """the check above can fail: pads whose msn follows their seq let zamboni run on"""
    batch = oracle_lib.generate(1, seed=rc.SEED, ops_per_doc=100, **rc.WORKLOADS['annotate'])
    good = rc.pad_tail(batch, 120)
    bad = rc.pad_tail(batch, 120)
    bad.ops['msn'][100:] = bad.ops['seq'][100:] - 1
    plain, a, b = (oracle_lib.Oracle(1).apply(x) for x in (batch, good, bad))
    assert _same_but_seq(plain.state(0), a.state(0)) and not _same_but_seq(plain.state(0), b.state(0))
    assert a.state(0)['msn'] == plain.state(0)['msn'] != b.state(0)['msn']
    _noop_at(plain, 120)
    assert int(plain.checksums()[0]) == int(a.checksums()[0]) != int(b.checksums()[0])


@pytest.mark.parametrize('fixture', rc.HALT_FIXTURES)
def test_padded_error_fixtures(oracle_lib, fixture):
    from conftest import load_golden
    from test_errors import ref_code
    batch, exp = load_golden(fixture)
    plain = oracle_lib.Oracle(batch.n_docs).apply(batch)
    for K in K_HALT:
        n = launch_size(K)
        padded, o, _ = rc.halts(fixture, K)
        assert np.diff(padded.row_ptr).tolist() == [n] * batch.n_docs
        for r in exp:
            d = r['doc']
            code = ref_code(r['err'])
            assert o.error(d) == ((code, r['err_seq']) if code else (0, 0)), (K, d)
            if code:  # a halted document ignores the padding
                assert o.state(d) == r['state'] and '%016x' % o.checksums()[d] == r['checksum'], (K, d)
            else:
                assert _same_but_seq(o.state(d), plain.state(d)) and o.text(d) == plain.text(d), (K, d)
            # a new document, n records, inside the offset window: class K on the register engine
            ops = padded.ops[int(padded.row_ptr[d]):int(padded.row_ptr[d + 1])]
            assert class_for(*FRESH, n) == K and rc.fits_window(ops, 0, 0), (K, d)


def _replay_with_budget(name, n):
    """the scenario op by op: (arena room left before each insert, the oracle)"""
    from oracle import oracle
    o = oracle.Oracle(1).record_events()
    room = []
    for b in rc.scenario_batches(name, n):
        for rec, part in zip(b.ops, b.split_ops(1)):
            if (int(rec['type']) & 7) == INSERT:
                room.append(ARENA - rc.linked_text(o, 0) - (int(rec['payload_len']) - 2 * ((int(rec['flags']) >> 3) & 15)))
            o.apply(part)
    return room, o


@pytest.mark.parametrize('name', ['A2', 'A3', 'A4', 'A5'])
def test_arena_scenarios_fit_their_arena(oracle_lib, name):
    """Before every insert, the text of every segment still in the tree (tombstones included) plus the
    insert's fits an arena half, and zamboni appends nothing (an append's copy needs room of its own):
    whatever the engine compacts, it finds the room -- no arena error is the only right outcome."""
    for n in (None, launch_size(7), launch_size(16)):
        room, o = _replay_with_budget(name, n)
        assert min(room) >= 0, (name, n, room)
        ops = [op for _, op, _ in o.events(0)]
        assert EV_APPEND not in ops and EV_UNLINK in ops, (name, n)
        _, ref = rc.scenario(name, n)
        assert o.state(0) == ref.state(0) and o.events(0) == ref.events(0)
    # the inserts after the first start from a full (or nearly full) half: each needs a compaction
    first = rc.SCENARIOS[name][0][0]
    assert len(first[4]) >= ARENA - 1


def test_the_removed_whole_arena_segment_is_unlinked_before_the_next_insert():
    """A3: the non-op messages' msn lets zamboni unlink each tombstone, and the following insert comes
    after that in the oracle's callbacks"""
    _, o = rc.scenario('A3')
    evs = [(seq, op, sum(s[2] for s in segs)) for seq, op, segs in o.events(0)]
    unlink = [i for i, e in enumerate(evs) if e[1] == EV_UNLINK]
    inserts = [i for i, e in enumerate(evs) if e[1] == EV_INSERT]
    assert [evs[i] for i in unlink] == [(3, EV_UNLINK, ARENA), (6, EV_UNLINK, 40000)]
    assert [evs[i][0] for i in inserts] == [1, 4, 7, 8]
    assert inserts[1] > unlink[0] and inserts[2] > unlink[1]


def test_a1_is_the_halt_of_the_whole_arena_test():
    (b,), o = rc.scenario('A1')
    assert b.ops['payload_len'].tolist() == [ARENA, 1] and b.ops['pos1'].tolist() == [0, 0]
    assert [s[0] for s in o.state(0)['segs']] == [rc.WHOLE] and o.state(0)['seq'] == 1
    (c,), _ = rc.scenario('A1', 64, rc.C64_SHIFT)
    assert c.ops['client'].min() > 32 and len(c.ops) == 64


# ---- B ----------------------------------------------------------------------------------------------
CASES = [(w, c) for w in sorted(rc.WORKLOADS) for c in sorted({rc.n_clients(w, f) for f in rc.FORMS})]


@pytest.mark.parametrize('name,clients', CASES)
def test_workloads_reach_their_classes(name, clients):
    """From the oracle's states at the start of every launch: each apply's documents are predicted into
    the class it is meant for or the one above, never past the register engine's largest, inside the
    offset window, and with the segment count the issue's bound allows."""
    reached = set()
    for step in rc.B_STEPS:
        batch, o, shapes = rc.workload(name, clients, step)
        n = rc.step_launch(step)
        per = np.diff(batch.row_ptr).tolist()
        assert per == [per[0]] * rc.N_DOCS and per[0] % n == 0 and per[0] <= 400
        assert step == 'small' or per[0] == 3 * n  # a new document, then two loads of a stored one
        if clients == rc.C64_CLIENTS:
            assert int(batch.ops['client'].max()) > 32
        pred = [[class_for(*sh, n) for sh in launch] for launch in shapes]
        want = {2, 3, 4} if step == 'small' else {step}
        got = {k for launch in pred for k in launch}
        assert want <= got and None not in got and got <= want | {max(want) + 1}, (name, clients, step, pred)
        if step != 'small':
            assert set(pred[0]) == {step}
            for launch in shapes:
                for nseg, _, _, _, n_empty in launch:
                    assert nseg <= 48 * step - 2 - n_empty, (name, clients, step, nseg)
        parts = batch.split_ops(n)
        for d in range(rc.N_DOCS):  # (generated logs: reference sequence numbers never fall below the msn)
            msn = 0
            for t, part in enumerate(parts):
                ops = part.ops[int(part.row_ptr[d]):int(part.row_ptr[d + 1])]
                assert rc.fits_window(ops, msn, 0), (name, clients, step, d, t)
                msn = int(ops['msn'].max())
        reached |= got
    assert set(K_ALL) <= reached


def test_mid_log_padding_moves_nothing(oracle_lib):
    """K = 15 / 16 replay the K = 5 log with non-ops at the current sequence number after every 40
    records: state (its seq included), text, events and checksum are the unpadded log's"""
    for name, clients in CASES:
        _, plain, _ = rc.workload(name, clients, 5)
        for K in rc.B_REAL:
            batch, padded, _ = rc.workload(name, clients, K)
            assert int((batch.ops['type'] == NOOP).sum()) >= rc.N_DOCS * 3 * (launch_size(K) - rc.B_REAL[K])
            for d in range(rc.N_DOCS):
                assert padded.state(d) == plain.state(d) and padded.events(d) == plain.events(d), (name, K, d)
            assert np.array_equal(padded.checksums(), plain.checksums())


@pytest.mark.parametrize('clients', [32, rc.C64_CLIENTS])
def test_churn_arenas_hold_twice_the_linked_text(oracle_lib, clients):
    """The churn documents' arena half is larger than twice the largest linked text -- twice what the
    largest document inserts, and the linked text at every launch's end is below that -- and as small as
    1 KiB steps allow.  The other bound test_gpu_compaction.py sets, an arena half below half the
    inserted bytes, cannot hold with it here: logs of at most 384 records do not turn their text over
    (with 32 clients the msn trails some hundred records, so nearly all that is inserted is still
    linked, tombstones included).  The compactions in every class come from the turnover documents
    below, whose arena meets both bounds."""
    for step in rc.B_STEPS:
        cap, most = rc.churn_arena(clients, step)
        assert 2 * most < cap <= 2 * most + 1024 and cap <= ARENA
        batch, _, _ = rc.workload('churn', clients, step)
        o, linked = oracle_lib.Oracle(rc.N_DOCS), 0
        for part in batch.split_ops(rc.step_launch(step)):
            o.apply(part, threads=4)
            linked = max([linked] + [rc.linked_text(o, d) for d in range(rc.N_DOCS)])
        assert most // 2 < linked <= most, (step, linked, most)


def test_turnover_documents_overflow_a_tight_arena():
    """the arena half is larger than twice the largest linked text and smaller than half of what every
    document inserts, as test_gpu_compaction.py asks of its documents; the documents stay small"""
    for K in range(5, 17):
        for shift in (0, rc.C64_SHIFT):
            batch, o, most = rc.turnover(K, shift)
            n = launch_size(K)
            assert np.diff(batch.row_ptr).tolist() == [3 * n] * rc.N_DOCS
            assert 2 * most < rc.TURN_ARENA
            assert all(rc.inserted_bytes(batch, d) > 2 * rc.TURN_ARENA for d in range(rc.N_DOCS)), K
            assert any(op == EV_APPEND for _, op, _ in o.events(0))
            ref = type(o)(rc.N_DOCS)
            for part in batch.split_ops(n):
                assert {class_for(*rc.doc_shape(ref, d), n) for d in range(rc.N_DOCS)} == {K}
                ref.apply(part)
