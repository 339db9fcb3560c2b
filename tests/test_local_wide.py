"""An editing client on a wide document (include/mtgpu.h "limits"): the fixtures' coverage and the record
encoding, on the CPU.

The fixtures come from the reference itself (tests/golden/make_localw.py: a farm of reference Clients,
logged as the editing client sees it, with UTF-16 text, keys 0..31, value ids up to 65535 and client ids
>= 64 and >= 256).  The CPU oracle keeps refusing editing-and-wide documents, so the GPU tests
(test_local_wide_gpu.py) compare with the reference's own states stored here."""
import numpy as np

import localw


def _non_latin(text):
    return any(ord(c) > 255 for c in text or '')


def test_fixture_covers_the_wide_editing_paths():
    from fluidframework_amd.oplog import ANNOTATE, F_REWRITE, INSERT, decode_record
    wide_local = non_latin = key8 = key16 = rewrites = 0
    pending_wide = pending_rm = 0
    summ = localw.summary()
    for name in localw.LOGS + [localw.LONG]:
        batch, rows = localw.load(name)
        for row in rows:
            a, b = int(batch.row_ptr[row['doc']]), int(batch.row_ptr[row['doc'] + 1])
            assert b - a == row['n'] and (name in ('localw_offline', localw.LONG) or row['n'] <= 400)
            for i in range(a, b):
                o = batch.ops[i]
                if o['seq'] != -1:
                    continue
                t, fl, text, props = decode_record(o, batch.payload)
                if t == ANNOTATE and fl & F_REWRITE:
                    rewrites += 1
                if not int(o['type']) & localw.OP_WIDE:
                    continue
                wide_local += 1
                non_latin += t == INSERT and _non_latin(text)
                key8 += t == ANNOTATE and any(k >= 8 for k in props)
                key16 += t == ANNOTATE and any(k >= 16 for k in props)
            for k, _, _, flags, _ in row['states'][:-1]:  # (the generator's flags of each state)
                pending_wide += 'w' in flags
                pending_rm += 'r' in flags
            # every local edit is acked by the end: nothing pending in the end state, and (without
            # reconnects) as many acks as edits
            assert row['states'][-1][3] == '', (name, row['doc'])
            if 'end' in row:
                assert not any(s[1] == -1 or (s[3] == -1 and s[4] != -1) for s in row['end']['segs']), (name, row['doc'])
            if name != 'localw_reconnect':
                assert localw.pending_edits(batch, row, row['n']) == 0, (name, row['doc'])
            assert 5 <= len(row['states']) <= 7, (name, row['doc'], len(row['states']))
    assert wide_local >= 300 and non_latin >= 100 and key8 >= 60 and key16 >= 15 and rewrites >= 10, \
        (wide_local, non_latin, key8, key16, rewrites)
    # the farm's own counts (what the records alone do not show: the editing client's pending counts
    # when a remote annotate arrives)
    over = sum(v['counts']['overPending'] for v in summ.values())
    dropped = sum(v['counts']['dropped'] for v in summ.values())
    assert over >= 40 and dropped >= 5, (over, dropped)
    assert pending_wide >= 40 and pending_rm >= 15, (pending_wide, pending_rm)
    batch, rows = localw.load('localw_reconnect')
    regen = [op for r in rows for _, ops in r['regen'] for op in ops]
    wide_regen = [op for op in regen if _non_latin(op[3]) or any(int(k) >= 8 for k in (op[4] or {}))]
    assert len(regen) >= 200 and len(wide_regen) >= 50, (len(regen), len(wide_regen))
    batch, rows = localw.load('localw_offline')
    assert len(rows) == 2
    for row in rows:
        assert max(localw.pending_edits(batch, row, k) for k, *_ in row['states']) > 64, row['doc']
    assert summ['localw_rounds']['dropped'] == 0 and summ['localw_rounds']['kept'] == 6
    for name, n in (('localw_lag', 6), ('localw_promote', 6), ('localw_own_hi', 3), ('localw_reconnect', 4)):
        assert len(localw.load(name)[1]) == n
    own = [r['ids'][0] for r in localw.load('localw_own_hi')[1]]
    assert sum(64 <= c < 256 for c in own) == 2 and sum(c >= 256 for c in own) == 1
    batch, rows = localw.load(localw.LONG)
    assert rows[0]['n'] >= 2100 and max(s[2] for s in rows[0]['states']) < 900


def test_promote_documents_turn_wide_with_edits_pending():
    """localw_promote: narrow up to the promoting record, which is the editing client's own wide edit
    (documents 0, 1), a remote wide op (2, 3) or an op of a client id >= 64 (4, 5); an edit is pending
    there, and a checkpoint sits on each side of it."""
    batch, rows = localw.load('localw_promote')
    assert [r['promote']['route'] for r in rows] == [0, 0, 1, 1, 2, 2]
    for row in rows:
        a, k, own = int(batch.row_ptr[row['doc']]), row['promote']['k'], row['ids'][0]
        assert not any(localw.wide_record(batch, a + i) for i in range(k)), row['doc']
        o = batch.ops[a + k]
        assert localw.wide_record(batch, a + k)
        assert [o['seq'] == -1 and o['type'] & localw.OP_WIDE, o['seq'] > 0 and o['client'] != own and o['type'] & localw.OP_WIDE,
                o['seq'] > 0 and o['client'] >= 64][row['promote']['route']]
        assert localw.pending_edits(batch, row, k) >= 1 and row['promote']['pending'] >= 1
        ks = [kk for kk, *_ in row['states']]
        assert k in ks and k + 1 in ks


def test_wide_records_round_trip():
    """A wide local record and a wide regenerated record through oplog.py's encoder and decoder: UTF-16
    text with a lone surrogate, 3-byte pairs, 24 pairs through MT_OP_NP16."""
    from fluidframework_amd.oplog import (ANNOTATE, F_MARKER, F_PROPS, F_REWRITE, INSERT, OP_NP16, OP_NP32, OP_WIDE,
                                          build_batch, decode_record, npairs)
    text = 'a日😀\ud83dzé'  # (a pair, then a lone high surrogate)
    p24 = {k: (65535 - k if k % 3 else None) for k in range(24)}
    docs = [[(-1, 0, 0, 300, INSERT, 0, 0, text, {9: 40000, 0: 7}, 0),
             (-1, 0, 0, 300, ANNOTATE, 0, 3, None, p24, F_REWRITE),
             (-1, 0, 0, 300, INSERT, 1, 0, '\x01', {7: 256}, F_MARKER),
             (-2, 0, 0, 300, ANNOTATE, 0, 2, None, {31: 65535}, 0),
             (-1, 0, 0, 300, INSERT, 0, 0, 'plain', None, 0)]]
    b = build_batch(docs)
    got = [decode_record(o, b.payload) for o in b.ops]
    assert got[0] == (INSERT, F_PROPS, text, {9: 40000, 0: 7})
    assert got[1] == (ANNOTATE, F_REWRITE, None, p24)
    assert got[2] == (INSERT, F_PROPS | F_MARKER, '\x01', {7: 256})
    assert got[3] == (ANNOTATE, 0, None, {31: 65535})
    assert got[4] == (INSERT, 0, 'plain', None)
    t = b.ops['type']
    assert all(t[:4] & OP_WIDE) and not t[4] & OP_WIDE
    assert t[1] & OP_NP16 and not t[1] & OP_NP32 and npairs(b.ops['flags'][1], t[1]) == 24
    units = len(text.encode('utf-16-le', 'surrogatepass')) // 2  # (7: the pair is two)
    assert b.ops['payload_len'][0] == 2 * units + 3 * 2 and b.ops['payload_len'][1] == 3 * 24
    assert np.array_equal(b.ops['client'], [300] * 5)
