"""findTile / getStackContext asked in the middle of editing, wide and observer logs:
the fixture and the CPU oracle.  tests/golden/tileforms.expected.jsonl holds what the reference's own
Client answered at checkpoints of the tf_* logs (tests/golden/make_tileforms.py): after every label
annotate, on both sides of the ack of the logged client's own label annotate, and spread over each log --
where a block's caches are still stale, which an end-of-log query mostly no longer sees.  Beside each answer
the fixture keeps the plain answer (a flat walk with the current labels) where it differs.  All comparisons
are exact."""
import os
import shutil
import sys

import pytest

import tileforms
from conftest import GOLDEN
from tileforms import LOGS

ANNOTATE, OP_WIDE, F_GROUP_MORE = 2, 0x80, 4


def records_of(batch, row):
    """[(seq, client, base type, wide, text, props)] of a row's document"""
    from fluidframework_amd.oplog import decode_record
    a = int(batch.row_ptr[row['doc']])
    out = []
    for r in batch.ops[a:a + row['n']]:
        t, fl, text, props = decode_record(r, batch.payload)
        out.append((int(r['seq']), int(r['client']), t & 7, bool(int(r['type']) & OP_WIDE), text, props or {}, fl))
    return out


def test_fixture_shape():
    head = tileforms.head()['counts']
    total = dict(stale=0, flips_farm=0, ptile=0, removed=0)
    for name in LOGS:
        batch, rows = tileforms.load(name)
        assert 4 <= len(rows) <= 6 and batch.n_docs == len(rows), name
        stale = flips = 0
        for row in rows:
            recs = records_of(batch, row)
            n, cks = row['n'], row['checkpoints']
            assert n == int(batch.row_ptr[row['doc'] + 1]) - int(batch.row_ptr[row['doc']])
            assert n <= 700 and len(cks) >= 8, (name, row['doc'], n, len(cks))
            ends = {0} | {i + 1 for i, r in enumerate(recs) if not r[6] & F_GROUP_MORE}
            ks = [ck['k'] for ck in cks]
            assert ks == sorted(set(ks)) and set(ks) <= ends and ks[-1] == n, (name, row['doc'])
            assert row['observer'] == (not any(r[0] < 0 for r in recs))
            # label value ids stay in 1..15 (None: the key deleted): the 256-bit vmask contract
            labels = [(i, r) for i, r in enumerate(recs) if any(k in row['keys'] for k in r[5])]
            assert all(r[5][k] is None or 1 <= r[5][k] <= 15 for _, r in labels for k in r[5] if k in row['keys'])
            # every label annotate is followed by a checkpoint with no structural op between
            for i, r in labels:
                if r[2] != ANNOTATE:
                    continue
                nxt = next((j for j in range(i + 1, n) if recs[j][2] in (0, 1)), n)
                assert any(i < k <= nxt for k in ks), (name, row['doc'], i)
            for q, ck in enumerate(cks):
                assert len(ck['pos']) <= 24 and ck['pos'] == sorted(set(ck['pos']))
                total['ptile'] += ck['ptile']
                total['removed'] += 1 if ck['removed'] else 0
                if 'check' in ck:
                    continue
                assert len(ck['tiles'][0]) == 8 * len(ck['pos']) and len(ck['stacks'][0]) == 4 * len(ck['pos'])
                # the two recorded columns: the plain one is kept where it differs
                for col in ('tiles', 'stacks'):
                    assert all(plain != ck[col][0][i] for i, plain in ck[col][1]), (name, row['doc'], ck['k'])
                    stale += len(ck[col][1])
                if ck['why'] == 'ack':
                    # the step holds the ack of a local label annotate and nothing else
                    step = recs[cks[q - 1]['k']:ck['k']]
                    assert step and all(r[0] > 0 and r[1] == row['ids'][0] and r[2] == ANNOTATE for r in step)
                    assert any(k in row['keys'] for r in step for k in r[5])
                    assert cks[q - 1]['len'] == ck['len'] and cks[q - 1]['pend'][1] == ck['pend'][1] + 1
                    flips += tileforms.flips(cks[q - 1], ck)
        assert stale > 0 and stale == head[name]['stale_differs_full'] <= head[name]['stale_differs'], (name, stale)
        total['stale'] += stale
        if name == 'tf_scenarios':
            assert flips > 0
        else:
            total['flips_farm'] += flips
    assert total['stale'] >= 100 and total['flips_farm'] > 0, total
    assert total['ptile'] > 0 and total['ptile'] == sum(h['pending_tile'] for h in head.values())
    assert total['removed'] > 0 and total['removed'] == sum(h['pending_removed'] for h in head.values())


def test_fixture_forms():
    """What sends each log to its form of the engine: editing clients, more than 64 edits pending, content
    past the narrow limits with the labels on keys 20 and 27, documents that turn wide with a label annotate
    of the editing client's own pending."""
    import json
    with open(os.path.join(GOLDEN, 'tileforms.summary.json')) as f:
        summary = json.load(f)
    assert set(summary) == set(LOGS) and all(s['kept'] + s['dropped'] == s['tried'] for s in summary.values())
    for name in LOGS:
        batch, rows = tileforms.load(name)
        for row in rows:
            recs = records_of(batch, row)
            wide = [i for i, r in enumerate(recs) if r[3] or (r[1] >= 64 and r[2] != 3)]
            if name in ('tf_wide', 'tf_edit_wide'):
                assert row['keys'] == [20, 27] and wide
                assert row['observer'] == (name == 'tf_wide')
                if row['promote']:
                    # narrow up to its own label annotate on key 20, which is pending at a checkpoint
                    k = row['promote']['k']
                    assert wide[0] == k and recs[k][0] == -1 and recs[k][2] == ANNOTATE and 20 in recs[k][5]
                    assert any(ck['k'] > k and ck['pend'][1] > 0 for ck in row['checkpoints'])
                else:
                    clients = {r[1] for r in recs}
                    assert any(64 <= c < 256 for c in clients) and any(c >= 256 for c in clients)
                    assert any(ord(ch) > 255 for r in recs for ch in (r[4] or '') if r[2] == 0 and not r[6] & 128)
                    assert any((v or 0) > 255 for r in recs for k, v in r[5].items() if k not in row['keys'])
            else:
                assert row['keys'] == [0, 1] and not wide
                assert row['observer'] == (row['name'] == 'scenario_f')
        if name == 'tf_edit_wide':
            assert sum(1 for r in rows if r['promote']) == 2
        if name == 'tf_edit_offline':
            assert all(r['counts']['pendingMax'] > 64 for r in rows)
            assert any(ck['pend'][0] > 64 for r in rows for ck in r['checkpoints'])
        if name == 'tf_edit_reconnect':
            assert sum(1 for r in rows for x in records_of(batch, r) if x[0] == -2) >= 10


HAVE_REF = os.path.isdir('/root/reference/packages/dds/merge-tree/src') and shutil.which('node') and \
    os.path.isdir(os.path.join(os.path.dirname(GOLDEN), '..', 'oracle', '_tsref'))


@pytest.mark.reference
@pytest.mark.skipif(not HAVE_REF, reason='reference sources / node / oracle/_tsref not present (GPU box)')
def test_fixture_regenerates_byte_identically(tmp_path):
    sys.path.insert(0, GOLDEN)
    import make_tileforms
    make_tileforms.main(str(tmp_path))
    for f in ('tileforms.expected.jsonl', 'tileforms.summary.json') + tuple(n + '.mtlog' for n in LOGS):
        with open(os.path.join(GOLDEN, f), 'rb') as a, open(tmp_path / f, 'rb') as b:
            assert a.read() == b.read(), f


def oracle_answers(o, i, row, ck):
    tk, rk = row['keys']
    tiles = [o.find_tile(i, p, tk, tileforms.MASKS[l], bool(prec)) for p, l, prec in tileforms.tile_asks(ck)]
    stacks = [o.stack_context(i, p, rk, tileforms.MASKS[l]) for p, l in tileforms.stack_asks(ck)]
    return tiles, stacks


@pytest.mark.parametrize('name', [n for n in LOGS if n != 'tf_edit_wide'])
def test_oracle_matches_reference(oracle_lib, name):
    """The CPU oracle follows each log checkpoint by checkpoint and answers every query as the reference did
    -- editing documents with edits pending included.  (tf_edit_wide: the oracle refuses editing-and-wide
    documents; only the reference pins them.)"""
    batch, rows = tileforms.load(name)
    o = oracle_lib.Oracle(len(rows))
    at = [0] * len(rows)
    asked = 0
    for cks in tileforms.steps(rows):
        hi = [ck['k'] if ck else a for ck, a in zip(cks, at)]
        if hi != at:
            o.apply(tileforms.span(batch, rows, at, hi))
        at = hi
        for i, (row, ck) in enumerate(zip(rows, cks)):
            if ck is None:
                continue
            assert o.error(i) == (0, 0), (name, row['doc'], ck['k'], o.error(i))
            bad = tileforms.same_answers(ck, *oracle_answers(o, i, row, ck))
            assert not bad, (name, row['doc'], ck['k'], ck['why'], bad[:3])
            asked += 12 * len(ck['pos'])
    assert at == [r['n'] for r in rows] and asked == tileforms.head()['counts'][name]['answers']


def test_oracle_refuses_editing_and_wide_documents(oracle_lib):
    """That stays as it is: tf_edit_wide halts in the oracle at its first wide record."""
    batch, rows = tileforms.load('tf_edit_wide')
    o = oracle_lib.Oracle(len(rows)).apply(tileforms.span(batch, rows, [0] * len(rows), [r['n'] for r in rows]))
    assert all(o.error(i)[0] != 0 for i in range(len(rows)))


@pytest.mark.parametrize('name', ['tf_edit', 'tf_wide'])
def test_padding_changes_no_answer(oracle_lib, name):
    """tileforms.padded (what test_tileforms_gpu.py::test_workspace_forms applies: each step behind no-op
    messages, one launch of 300 records): the oracle's answers at every checkpoint of the log's first
    document are still the reference's."""
    batch, rows = tileforms.load(name)
    row = rows[0]
    o = oracle_lib.Oracle(1)
    at = 0
    for ck in row['checkpoints']:
        step = tileforms.padded(batch, row, at, ck['k'], 300)
        assert step.n_ops == 300
        o.apply(step)
        at = ck['k']
        assert o.error(0) == (0, 0), (name, ck['k'], o.error(0))
        bad = tileforms.same_answers(ck, *oracle_answers(o, 0, row, ck))
        assert not bad, (name, ck['k'], bad[:3])
