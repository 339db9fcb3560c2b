"""Remote views (refSeq, client) with client ids >= 64 and >= 256 in every read kernel:
mt_resolve_positions, mt_text_ranges / mt_text_lengths and mt_marker_positions all answer through
csrc/mt_view.h, and mt_fixup_kernel restates the rule to rank "MergeTree insert failed" against the
window asserts.  tests/view_docs.py holds the documents (the reference's final states of the wide
goldens, and hand-made logs whose states come from the CPU oracle), the plan of views and the plain
rule; here the plan is shown to tell the correct reader from four wrong ones (CPU), and the kernels
are asked every view of it (GPU).  All comparisons are exact."""
import numpy as np
import pytest

import view_docs as vd


@pytest.fixture(scope='module')
def suite(oracle_lib):
    return vd.Suite(oracle_lib)


# ---- CPU ------------------------------------------------------------------------------------------
def test_view_plan_covers_every_class(suite, oracle_lib):
    """Every class of the plan's table holds (segment, view) pairs, and every class a wrong reader can
    reach holds pairs on which one of view_docs.WRONG answers differently from the rule; for the classes
    none of the four can reach (view_docs.UNTOUCHED says why) the count alone.  No document of the plan
    errs in the oracle but H3's, which err as intended."""
    pairs = {k: 0 for k in vd.CLASSES}
    told = {k: 0 for k in vd.CLASSES}
    by_rule = {w: 0 for w in vd.WRONG}
    n_views = 0
    for k in range(2):
        for d in range(suite.n_docs):
            assert suite.errors[k][d] == (0, 0), (suite.labels[d], k)
            if k and not suite.second_state(d):
                continue
            views = suite.plan(k, d)
            n_views += len(views)
            assert all(r is None or r >= suite.states[k][d]['msn'] for r, _ in views)
            p, t, b = vd.class_counts(suite.states[k][d], views)
            for c in vd.CLASSES:
                pairs[c] += p[c]
                told[c] += t[c]
                for w in vd.WRONG:
                    by_rule[w] += b[c][w]
    print('\nviews: %d; (segment, view) pairs per class, and those a wrong reader answers differently:' % n_views)
    for c in vd.CLASSES:
        print('  %-20s %7d %6d' % (c, pairs[c], told[c]))
    print('  told per wrong reader (a pair counts once per class it is in):', by_rule)
    for c in vd.CLASSES:
        assert pairs[c] > 0, c
        if c in vd.UNTOUCHED:
            assert told[c] == 0, c
        else:
            assert told[c] > 0, c
    assert all(n > 0 for n in by_rule.values()), by_rule
    assert 500 < n_views < 5000
    # H0a: the hidden leaves cover ordinals 58..70 for the removers, the removed marker among them
    h0 = suite.states[0][suite.labels.index('h0')]
    hid = [i for i, s in enumerate(h0['segs']) if vd.view_len(s, 140, 500) == 0]
    assert hid == list(range(58, 71)) and isinstance(h0['segs'][64][0], dict)
    assert sorted(vd.high_members(h0['segs'][60][5])) == sorted(vd.H0_OVERLAP) and h0['segs'][60][4] == vd.H0_FIRST
    # H0b: zamboni has unlinked the removed ranges
    assert not any(s[4] != -1 for s in suite.states[1][suite.labels.index('h0')]['segs'])
    # H3
    want = {'h3_overlap_hi_past': 3, 'h3_overlap_hi_inside': 1, 'h3_remover_256_past': 3, 'h3_stranger_past': 1}
    for label, batch in vd.error_docs():
        o = oracle_lib.Oracle(1).apply(batch)
        assert o.error(0) == (want[label], int(batch.ops[-1]['seq'])), label
        assert o.state(0) == h0, label


def test_oracle_final_states_are_the_reference_states(suite):
    for i, st in suite.golden.items():
        assert suite.oracle_final[i] == st, suite.labels[i]
    # the material the issue counted: removed segments whose overlap sets hold ids >= 64
    n = {suite.labels[i]: sum(1 for s in st['segs'] if s[4] != -1 and vd.high_members(s[5]))
         for i, st in suite.golden.items()}
    assert n['wide[2]'] == 9 and n['wide_many[0]'] == 13 and n['wide_xl[0]'] == 18, n
    xl = suite.golden[suite.labels.index('wide_xl[0]')]
    assert sum(1 for s in xl['segs'] if len(vd.high_members(s[5])) > 16) == 14


def test_the_restatements_of_the_rule_agree(suite):
    """view_docs.view_len, textread.view_len and relpos.view_len are one rule; expected_table is
    `expected` at every position."""
    from fluidframework_amd import relpos, textread
    for d in range(suite.n_docs):
        st = suite.states[0][d]
        views = suite.plan(0, d)
        for r, c in views[::7] + views[:3]:
            for s in st['segs']:
                want = vd.view_len(s, r, c)
                assert textread.view_len(s, r, c) == want and relpos.view_len(s, r, c) == want, (suite.labels[d], r, c, s)
        for r, c in views[1::max(1, len(views) // 3)]:
            pos, o, f, p, ln = vd.expected_table(st, r, c)
            for k in list(range(0, len(pos), max(1, len(pos) // 9))) + [0, len(pos) - 2, len(pos) - 1]:
                assert (int(o[k]), int(f[k]), int(p[k]), int(ln[k])) == vd.expected(st, int(pos[k]), r, c)


# ---- GPU ------------------------------------------------------------------------------------------
def stages(suite, b):
    """(stage, engine) with the engine's documents at the stage's states, checked first: a read failure
    is then no apply failure in disguise"""
    from fluidframework_amd.engine import MergeEngine
    eng = MergeEngine(suite.n_docs, ops_per_launch=b)
    try:
        for k in range(2):
            eng.apply(suite.stage(k))
            for d in range(suite.n_docs):
                assert eng.error(d) == (0, 0), (suite.labels[d], k, b)
                assert eng.state(d) == suite.states[k][d], (suite.labels[d], k, b)
            yield k, eng
    finally:
        eng.close()


def shuffled(n, seed):
    return np.random.default_rng(seed).permutation(n)


def position_queries(suite, k):
    """every view of stage k: POS_CONTAINING at -1 .. the view's length + 1, POS_OF_ORDINAL of every
    ordinal and of n.  (queries, wanted (n, 4) int array), interleaved across views and documents."""
    from fluidframework_amd.engine import POS_CONTAINING, POS_LOCAL, POS_OF_ORDINAL, POS_QUERY_DTYPE
    qs, ws = [], []
    for d, r, c in suite.views(k):
        st = suite.states[k][d]
        n = len(st['segs'])
        pos, o, f, p, ln = vd.expected_table(st, r, c)
        vlen = len(pos) - 3
        q = np.zeros(len(pos) + n + 1, dtype=POS_QUERY_DTYPE)
        q['doc'], q['ref_seq'], q['client'] = d, POS_LOCAL if r is None else r, c
        q['pos'][:len(pos)] = pos
        q['kind'][:len(pos)] = POS_CONTAINING
        q['pos'][len(pos):] = np.arange(n + 1)
        q['kind'][len(pos):] = POS_OF_ORDINAL
        loc = np.array([vd.view_len(s, None, 0) for s in st['segs']], dtype=np.int64)
        un = np.array([vd.units(s[0]) for s in st['segs']], dtype=np.int64)
        w = np.zeros((len(q), 4), dtype=np.int64)
        w[:len(pos)] = np.stack([o, f, p, ln], axis=1)
        w[len(pos):-1] = np.stack([np.arange(n), np.zeros(n, np.int64), np.cumsum(loc) - loc, un], axis=1)
        w[-1] = (-1, n - vlen, loc.sum(), 0)   # no such ordinal: pos minus the view's length, the local length
        qs.append(q)
        ws.append(w)
    q, w = np.concatenate(qs), np.concatenate(ws)
    perm = shuffled(len(q), 11 + k)
    return q[perm], w[perm]


@pytest.mark.gpu
@pytest.mark.parametrize('b', [32, 7])
def test_positions_in_remote_views(suite, b):
    from fluidframework_amd.engine import POS_RESULT_DTYPE
    from fluidframework_amd.hipmem import DeviceBuffer
    total = 0
    for k, eng in stages(suite, b):
        q, want = position_queries(suite, k)
        got = eng.resolve_positions(q)
        g = np.stack([got['ordinal'], got['offset'], got['position'], got['length']], axis=1).astype(np.int64)
        bad = np.nonzero((g != want).any(axis=1))[0]
        if len(bad):
            i = bad[0]
            pytest.fail('%d of %d queries differ (b=%d, stage %d); the first: %s of %s -> %s, the state gives %s' % (
                len(bad), len(q), b, k, tuple(q[i]), suite.labels[int(q[i]['doc'])], tuple(g[i]), tuple(want[i])))
        sub = shuffled(len(q), 5)[:4096]
        dq, dr = DeviceBuffer(q[sub].nbytes).upload(q[sub]), DeviceBuffer(len(sub) * POS_RESULT_DTYPE.itemsize)
        eng.resolve_positions_device(dq.ptr, len(sub), dr.ptr)
        assert (dr.download(POS_RESULT_DTYPE) == got[sub]).all(), (b, k)
        total += len(q)
    assert total > 100000


def hidden_run_edges(st, r, c):
    """view positions of the first and of the longest run of leaves hidden in the view"""
    runs, p, i, segs = [], 0, 0, st['segs']
    while i < len(segs):
        if vd.view_len(segs[i], r, c) == 0:
            j = i
            while j < len(segs) and vd.view_len(segs[j], r, c) == 0:
                j += 1
            runs.append((j - i, p))
            i = j
        else:
            p += vd.view_len(segs[i], r, c)
            i += 1
    return sorted({runs[0][1], max(runs)[1]}) if runs else []


def text_queries(suite, k):
    """every view of stage k: the whole view, and ranges that start or end inside, at and one unit to
    either side of a hidden run, without a placeholder, and with one and TEXT_MARKERS.
    [(doc, start, end, ref_seq | None, client, placeholder, flags)]"""
    from fluidframework_amd.textread import TEXT_MARKERS
    rows = []
    for d, r, c in suite.views(k):
        st = suite.states[k][d]
        vlen = sum(vd.view_len(s, r, c) for s in st['segs'])
        ranges = [(0, vlen), (0, vlen + 5)]
        for p in hidden_run_edges(st, r, c):
            for e in (p - 1, p, p + 1):
                ranges += [(0, e), (e, vlen), (e, e + 2), (e - 3, e)]
        for n, (a, e) in enumerate(ranges):
            for ph, fl in (('', 0), ('#', TEXT_MARKERS)) if n < 2 else ((('', 0),) if n % 2 else (('#', TEXT_MARKERS),)):
                rows.append((d, a, e, r, c, ph, fl))
    return [rows[i] for i in shuffled(len(rows), 23 + k)]


@pytest.mark.gpu
@pytest.mark.parametrize('b', [32, 7])
def test_text_in_remote_views(suite, b):
    from fluidframework_amd import textread
    from fluidframework_amd.engine import MergeEngine
    from fluidframework_amd.hipmem import DeviceBuffer
    total = 0
    for k, eng in stages(suite, b):
        views = suite.views(k)
        # getLength(refSeq, clientId): the count pass over the whole range with a placeholder
        lq = MergeEngine.text_queries([d for d, _, _ in views], 0, None,
                                      [textread.TEXT_LOCAL if r is None else r for _, r, _ in views],
                                      [c for _, _, c in views], '#')
        lens = eng.text_lengths(lq)
        for (d, r, c), g in zip(views, lens):
            assert int(g['units']) == textread.get_length(suite.states[k][d]['segs'], r, c), (suite.labels[d], r, c, b, k)
        rows = text_queries(suite, k)
        q = MergeEngine.text_queries([x[0] for x in rows], [x[1] for x in rows], [x[2] for x in rows],
                                     [textread.TEXT_LOCAL if x[3] is None else x[3] for x in rows], [x[4] for x in rows],
                                     [x[5] for x in rows], [x[6] for x in rows])
        texts, marks = eng.text_ranges(q)
        for (d, a, e, r, c, ph, fl), t, m in zip(rows, texts, marks):
            wt, wm = textread.get_text(suite.states[k][d]['segs'], a, e, r, c, ph)
            assert t == wt and m == (wm if fl else []), (suite.labels[d], a, e, r, c, ph, fl, b, k)
        # a shuffled sub-batch through the device form: its count pass
        sub = shuffled(len(q), 7)[:2048]
        dq = DeviceBuffer(q[sub].nbytes).upload(q[sub])
        dc = DeviceBuffer(len(sub) * textread.TEXT_COUNT_DTYPE.itemsize)
        eng.text_ranges_device(dq.ptr, len(sub), 0, 0, 0, 0, dc.ptr)
        cnt = dc.download(textread.TEXT_COUNT_DTYPE)
        units = [len(textread.units(texts[i])) for i in sub]
        assert [int(x) for x in cnt['units']] == units, (b, k)
        assert [int(x) for x in cnt['markers']] == [len(marks[i]) for i in sub], (b, k)
        # and its write pass, into rows of the counted sizes
        rp = np.concatenate([[0], np.cumsum(cnt['units'])]).astype(np.uint32)
        mrp = np.concatenate([[0], np.cumsum(cnt['markers'])]).astype(np.uint32)
        drp, dmrp = DeviceBuffer(rp.nbytes).upload(rp), DeviceBuffer(mrp.nbytes).upload(mrp)
        du = DeviceBuffer(max(2, 2 * int(rp[-1])))
        dm = DeviceBuffer(max(8, textread.TEXT_MARKER_DTYPE.itemsize * int(mrp[-1])))
        eng.text_ranges_device(dq.ptr, len(sub), drp.ptr, du.ptr, dmrp.ptr, dm.ptr, dc.ptr)
        u = du.download(np.dtype('<u2'))[:int(rp[-1])]
        mk = dm.download(textread.TEXT_MARKER_DTYPE)[:int(mrp[-1])]
        for j, i in enumerate(sub):
            assert textread.from_units(u[rp[j]:rp[j + 1]]) == texts[i], (b, k, rows[i])
            assert [(int(x['ordinal']), int(x['out_offset'])) for x in mk[mrp[j]:mrp[j + 1]]] == marks[i], (b, k, rows[i])
        total += len(rows)
    assert total > 5000


@pytest.mark.gpu
@pytest.mark.parametrize('b', [32, 7])
def test_marker_positions_in_remote_views(suite, b):
    """H0's three markers (before, inside and after the removed range) and an id naming no marker, in
    every view of every document: the other documents hold no marker of that id and must say so."""
    from fluidframework_amd import relpos
    from fluidframework_amd.engine import (MARKER_QUERY_DTYPE, MARKER_RESULT_DTYPE, MKF_HIDDEN, MKF_TOMBSTONE,
                                           POS_LOCAL)
    from fluidframework_amd.hipmem import DeviceBuffer
    total = named = 0
    for k, eng in stages(suite, b):
        rows = [(d, r, c, v) for d, r, c in suite.views(k) for v in vd.MARKER_IDS]
        rows = [rows[i] for i in shuffled(len(rows), 31 + k)]
        q = np.zeros(len(rows), dtype=MARKER_QUERY_DTYPE)
        for i, (d, r, c, v) in enumerate(rows):
            q[i] = (d, POS_LOCAL if r is None else r, c, vd.MARKER_KEY, 0, v, 0)
        got = eng.marker_positions(q)
        for (d, r, c, v), g in zip(rows, got):
            st = suite.states[k][d]
            m = relpos.choose_marker(st, vd.MARKER_KEY, v)
            at = (suite.labels[d], r, c, v, b, k)
            ans = tuple(int(g[x]) for x in ('ordinal', 'position', 'flags', 'length'))
            if m is None:
                assert ans == (-1, 0, 0, 0), at
            else:
                seg = st['segs'][m]
                flags = (MKF_HIDDEN if vd.view_len(seg, r, c) == 0 else 0) | (MKF_TOMBSTONE if seg[4] != -1 else 0)
                assert ans == (m, relpos.marker_position(st, m, r, c), flags, 1), at
                named += 1
            for before, offset in ((False, 0), (True, 1), (False, 2)):
                rel = dict(key=vd.MARKER_KEY, value=v, before=before, offset=offset)
                mine = -1 if ans[0] < 0 else relpos.position_of(ans[1], ans[3], before, offset)
                assert mine == relpos.pos_from_relative(st, rel, r, c), at
        sub = shuffled(len(q), 3)[:2048]
        dq, dr = DeviceBuffer(q[sub].nbytes).upload(q[sub]), DeviceBuffer(len(sub) * MARKER_RESULT_DTYPE.itemsize)
        eng.marker_positions_device(dq.ptr, len(sub), dr.ptr)
        assert (dr.download(MARKER_RESULT_DTYPE) == got[sub]).all(), (b, k)
        total += len(rows)
    assert total > 3000 and named > 700


@pytest.mark.gpu
@pytest.mark.parametrize('b', [32, 7])
def test_insert_failed_precedence_for_high_ids(suite, oracle_lib, b):
    """H3: an insert that trips a window assert, sent by a client in the hi words of the overlap list, by
    a removedClient >= 256 and by a stranger 256 above a member: "insert failed" wins exactly when the
    position is past the end of the sender's own view (mt_fixup_kernel's reading of it)."""
    from fluidframework_amd.engine import MergeEngine
    from fluidframework_amd.oplog import OpBatch
    docs = vd.error_docs()
    batch = OpBatch.concat([x[1] for x in docs])
    o = oracle_lib.Oracle(len(docs)).apply(batch)
    eng = MergeEngine(len(docs), ops_per_launch=b)
    eng.apply(batch)
    try:
        for d, (label, _) in enumerate(docs):
            assert o.error(d)[0] in (1, 3)
            assert eng.error(d) == o.error(d), (label, b)
            assert eng.state(d) == o.state(d), (label, b)
        assert sorted(o.error(d)[0] for d in range(len(docs))) == [1, 1, 3, 3]
    finally:
        eng.close()
