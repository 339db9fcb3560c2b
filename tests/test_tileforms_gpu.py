"""findTile (mt_find_tiles) and getStackContext (mt_range_stacks) on editing, wide and big documents, asked
in the middle of their logs.  Both kernels answer from state the apply engine keeps per marker -- MT_SF_STALE
and `slab`, the label value ids a leaf block's caches held at its last blockUpdate -- and every form of the
LDS engine keeps it in its own way: the narrow observer form in LDS, the editing forms in HBM by slot, the wide
forms through `pval` over 32 keys and u16 value ids, the HBM-workspace forms by ordinal around every launch.
Wrong bookkeeping there changes no checksum, no state and no event; only these queries see it, and only
while the block is still stale.

Pinned by the reference itself: tests/golden/tileforms.expected.jsonl (tests/golden/make_tileforms.py) holds
what the reference's Client answered at checkpoints of the tf_* logs; the engine follows each log checkpoint
by checkpoint and must answer every query exactly the same.  The hand-built big and wave-boundary documents
are compared with the CPU oracle, which test_tileforms.py holds to the same fixture."""
import numpy as np
import pytest

import tileforms
from tileforms import CLASS_EDITING, CLASS_FLAGS, CLASS_GROUPS, CLASS_LDS, CLASS_WIDE, LOGS, MASKS

pytestmark = pytest.mark.gpu


def used_classes(eng):
    return {cap for cap, _, launches, _ in eng.last_class_stats() if launches}


def engine_answers(eng, asks):
    """asks: [(engine document, tile key, range key, [position, ...])] -> per ask (tiles, stacks) in the
    fixture's form: tiles per position, per label, preceding then not (position | None); stacks per position,
    per label ([[marker position, refType], ...]).  One batch of each kind; stacks with cap=2, so deeper
    ones take the re-ask path."""
    from fluidframework_amd.engine import TILE_QUERY_DTYPE
    tq, sq = [], []
    for d, tk, rk, pos in asks:
        for p in pos:
            for l in range(4):
                for prec in (1, 0):
                    tq.append((d, p, tk, prec, 0, 0, MASKS[l].view('<u4'), 0))
                sq.append((d, p, rk, 0, 0, 0, MASKS[l].view('<u4'), 0))
    if not tq:
        return []
    tiles = [None if g < 0 else int(g) for g in eng.find_tiles(np.array(tq, dtype=TILE_QUERY_DTYPE))['pos']]
    stacks = [[[int(x['pos']), int(x['ref_type'])] for x in s]
              for s in eng.range_stacks(np.array(sq, dtype=TILE_QUERY_DTYPE), cap=2)]
    out, t, s = [], 0, 0
    for _, _, _, pos in asks:
        out.append((tiles[t:t + 8 * len(pos)], stacks[s:s + 4 * len(pos)]))
        t += 8 * len(pos)
        s += 4 * len(pos)
    return out


def declare_keys(eng, rows):
    for i, r in enumerate(rows):
        eng.set_label_keys(r['keys'][0], r['keys'][1], doc=i)


@pytest.mark.parametrize('b', [1, 7, 32])
@pytest.mark.parametrize('name', LOGS)
def test_engine_matches_reference(name, b):
    """Every checkpoint of every document of the log, at launches of b records: all answers equal the
    reference's, no document halts, and the class statistics show that the form the log is meant for ran."""
    from fluidframework_amd.engine import MergeEngine
    batch, rows = tileforms.load(name)
    eng = MergeEngine(len(rows), ops_per_launch=b)
    declare_keys(eng, rows)
    at, seen, asked = [0] * len(rows), set(), 0
    for cks in tileforms.steps(rows):
        hi = [ck['k'] if ck else a for ck, a in zip(cks, at)]
        if hi != at:
            eng.apply(tileforms.span(batch, rows, at, hi))
            seen |= used_classes(eng)
        at = hi
        live = [(i, r, ck) for i, (r, ck) in enumerate(zip(rows, cks)) if ck is not None]
        for i, r, ck in live:
            assert eng.error(i) == (0, 0), (name, r['doc'], ck['k'], eng.error(i))
            assert eng.length(i) == ck['len'], (name, r['doc'], ck['k'])
        got = engine_answers(eng, [(i, r['keys'][0], r['keys'][1], ck['pos']) for i, r, ck in live])
        for (i, r, ck), (tiles, stacks) in zip(live, got):
            bad = tileforms.same_answers(ck, tiles, stacks)
            assert not bad, (name, b, r['doc'], ck['k'], ck['why'], ck['pend'], bad[:3])
            asked += len(tiles) + len(stacks)
    eng.close()
    assert at == [r['n'] for r in rows] and asked == tileforms.head()['counts'][name]['answers']
    hexes = [hex(c) for c in sorted(seen)]
    if name == 'tf_scenarios':
        assert any(c & CLASS_EDITING for c in seen) and any(c & CLASS_LDS for c in seen), hexes
    if name.startswith('tf_edit'):
        assert any(c & CLASS_EDITING for c in seen), hexes
    if name == 'tf_edit_offline':
        assert any(c & CLASS_EDITING and c & CLASS_GROUPS for c in seen), hexes
    if name == 'tf_wide':
        assert any(c & CLASS_WIDE and not c & CLASS_EDITING for c in seen), hexes
    if name == 'tf_edit_wide':
        assert any(c & CLASS_EDITING and c & CLASS_WIDE for c in seen), hexes
    else:
        assert not any(c & CLASS_EDITING and c & CLASS_WIDE for c in seen), hexes


@pytest.mark.parametrize('b', [300, 1000])
@pytest.mark.parametrize('name', ['tf_edit', 'tf_wide'])
def test_workspace_forms(name, b):
    """The first document of tf_edit and of tf_wide on an engine of 8192 segments, every step one launch of
    b records (tileforms.padded: the step's records behind no-op messages that change nothing, so the
    reference's answers stand).  mt_bin_kernel picks the smallest class with interior blocks + nops + 1 <=
    CAP / 8 + 8 (the rule quoted in test_local_wide_gpu.py::test_long_document_in_every_form): 300 records
    need 301 -- past the 2048 class's 264, the 4096-slot HBM-workspace form; 1000 need 1001 -- past 520, the
    8192-slot form.  Every launch runs at that capacity; tf_edit in the editing form from its first local
    edit on, tf_wide in the wide form from its first wide record on."""
    from fluidframework_amd.engine import MergeEngine
    batch, rows = tileforms.load(name)
    row = rows[0]
    cap = {300: 4096, 1000: 8192}[b]
    form = {'tf_edit': CLASS_EDITING, 'tf_wide': CLASS_WIDE}[name] | cap
    eng = MergeEngine(1, seg_capacity=8192, ops_per_launch=b)
    declare_keys(eng, [row])
    at, seen = 0, []
    for ck in row['checkpoints']:
        eng.apply(tileforms.padded(batch, row, at, ck['k'], b))
        used = used_classes(eng)
        assert len(used) == 1 and {c & ~CLASS_FLAGS for c in used} == {cap}, (name, b, ck['k'], [hex(c) for c in used])
        seen += used
        at = ck['k']
        assert eng.error(0) == (0, 0) and eng.length(0) == ck['len'], (name, b, ck['k'], eng.error(0))
        (tiles, stacks), = engine_answers(eng, [(0, row['keys'][0], row['keys'][1], ck['pos'])])
        bad = tileforms.same_answers(ck, tiles, stacks)
        assert not bad, (name, b, ck['k'], ck['why'], bad[:3])
    eng.close()
    # once in its form the document stays there, and most checkpoints are asked there
    first = seen.index(form)
    assert seen[first:] == [form] * (len(seen) - first) and first <= 2, (name, b, [hex(c) for c in seen])


# ---- hand-built documents against the CPU oracle ---------------------------------------------------

TILE, BEGIN, END = 1, 2, 4


def leaves(n, kinds, first_seq=1):
    """n leaves by alternating clients 1 and 2 at msn 0 (none is appended to its neighbour): leaf i is text
    of 1-3 units, or where kinds has i -- (refType, label mask) -- a marker whose labels are on key 0 (a Tile)
    or key 1 (a NestBegin / NestEnd).  Returns (records, position of every leaf)."""
    from fluidframework_amd.oplog import F_MARKER, INSERT
    ops, at, pos = [], [], 0
    for i in range(n):
        s = first_seq + i
        at.append(pos)
        if i in kinds:
            rt, mask = kinds[i]
            ops.append((s, s - 1, 0, 1 + i % 2, INSERT, pos, 0, chr(rt), {0 if rt == TILE else 1: mask}, F_MARKER))
            pos += 1
        else:
            t = ''.join(chr(97 + (i + j) % 26) for j in range(1 + i % 3))
            ops.append((s, s - 1, 0, 1 + i % 2, INSERT, pos, 0, t, None, 0))
            pos += len(t)
    at.append(pos)
    return ops, at


def every_seventh(n, forced):
    """Markers at every seventh leaf -- Tile, NestBegin, NestEnd in turn, a begin and the end after it under
    the same label so stacks stay shallow -- and at the leaves of `forced` {leaf: refType}."""
    kinds = {}
    for j, i in enumerate(range(0, n, 7)):
        rt = (TILE, BEGIN, END)[j % 3]
        kinds[i] = (rt, 1 + (j // 3) % 15 if rt == TILE else 1 << ((j // 3) % 4))
    for i, rt in forced.items():
        kinds[i] = (rt, 1 + i % 15 if rt == TILE else 1 << (i % 4))
    return kinds


def relabel(kinds, at, i, seq, client, own=False):
    """An annotate of marker i's labels to another mask: sequenced, or (own) the client's local edit."""
    from fluidframework_amd.oplog import ANNOTATE
    rt, mask = kinds[i]
    new = (mask % 15) + 1 if rt == TILE else 1 << ((mask.bit_length()) % 4)
    head = (-1, 0, 0) if own else (seq, seq - 1, 0)
    return head + (client, ANNOTATE, at[i], at[i] + 1, None, {0 if rt == TILE else 1: new}, 0)


def ask_everywhere(eng, o, d, what):
    """Every position 0 .. length + 1 of document d, all four labels, both directions, and the stacks: the
    engine's answers equal the oracle's."""
    n = eng.length(d)
    pos = list(range(n + 2))
    (tiles, stacks), = engine_answers(eng, [(d, 0, 1, pos)])
    want_t = [o.find_tile(d, p, 0, MASKS[l], bool(prec)) for p, l, prec in tileforms.tile_asks(dict(pos=pos))]
    want_s = [o.stack_context(d, p, 1, MASKS[l]) for p, l in tileforms.stack_asks(dict(pos=pos))]
    bad = [(i, tiles[i], want_t[i]) for i in range(len(want_t)) if tiles[i] != want_t[i]]
    assert not bad, (what, 'tiles', len(bad), bad[:5])
    bad = [(i, stacks[i], want_s[i]) for i in range(len(want_s)) if stacks[i] != want_s[i]]
    assert not bad, (what, 'stacks', len(bad), bad[:5])
    return sum(t is not None for t in want_t), sum(1 for s in want_s if s)


def both(n_docs, **kw):
    from fluidframework_amd.engine import MergeEngine
    from oracle import oracle
    oracle.build()
    eng = MergeEngine(n_docs, **kw)
    eng.set_label_keys(0, 1)
    return eng, oracle.Oracle(n_docs)


def apply_both(eng, o, docs):
    from fluidframework_amd.oplog import build_batch
    batch = build_batch(docs)
    eng.apply(batch)
    o.apply(batch)
    for d in range(len(docs)):
        assert eng.error(d) == (0, 0) and o.error(d)[0] == 0, (d, eng.error(d), o.error(d))
    assert np.array_equal(eng.checksums()[:len(docs)], o.checksums()[:len(docs)])
    return used_classes(eng)


def big_observer_document():
    """An observer document of 2,300 leaves on an engine of 4096 segments (a workspace class): label annotates
    on the markers at ordinals 63, 64, 65, 127, 128 and on the last marker leave their blocks stale; asked
    everywhere, and again after one insert into the first block refreshes that block alone."""
    from fluidframework_amd.oplog import INSERT
    n = 2300
    kinds = every_seventh(n, {63: TILE, 64: BEGIN, 65: END, 127: TILE, 128: BEGIN})
    ops, at = leaves(n, kinds)
    eng, o = both(1, seg_capacity=4096, ops_per_launch=32)
    used = apply_both(eng, o, [ops])
    assert max(c & ~CLASS_FLAGS for c in used) == 4096, [hex(c) for c in used]
    s = n
    ann = []
    for i in (63, 64, 65, 127, 128, max(kinds)):
        s += 1
        ann.append(relabel(kinds, at, i, s, 1 + s % 2))
    used = apply_both(eng, o, [ann])
    assert {c & ~CLASS_FLAGS for c in used} == {4096}, [hex(c) for c in used]
    found, deep = ask_everywhere(eng, o, 0, 'after the annotates')
    assert found > 20000 and deep > 1000
    apply_both(eng, o, [[(s + 1, s, 0, 1, INSERT, 1, 0, 'ins', None, 0)]])
    ask_everywhere(eng, o, 0, 'after the insert')
    eng.close()


def big_editing_document():
    """An editing document grown past 1,024 segments the same way (the 2048-slot HBM-workspace editing form):
    its client's label annotates of the markers at ordinals 63, 64 and 128 pending, asked everywhere before
    and after each ack."""
    n = 1100
    kinds = every_seventh(n, {63: TILE, 64: BEGIN, 65: END, 127: TILE, 128: BEGIN})
    ops, at = leaves(n, kinds)
    eng, o = both(1, seg_capacity=4096, ops_per_launch=32)
    mine = [relabel(kinds, at, i, 0, 3, own=True) for i in (63, 64, 128)]
    used = apply_both(eng, o, [ops + mine])
    assert CLASS_EDITING | 2048 in used, [hex(c) for c in used]
    ask_everywhere(eng, o, 0, 'pending')
    for j, rec in enumerate(mine):
        s = n + 1 + j
        used = apply_both(eng, o, [[(s, n, 0) + rec[3:]]])
        assert used == {CLASS_EDITING | 2048}, [hex(c) for c in used]
        ask_everywhere(eng, o, 0, 'after ack %d' % j)
    eng.close()


def test_big_documents_against_oracle():
    """No reference run: two hand-built documents against the oracle at every position, all four labels and
    both directions (thousands of queries in one batch)."""
    big_observer_document()
    big_editing_document()


def test_single_block_documents_past_the_end():
    """Documents of at most eight leaves: the root is the only block, so a query at or past the length
    shifts over leaves, which answer with their current labels -- also a relabelled one (observer documents,
    and an editing client's own relabel pending, then acked)."""
    docs = []
    for n in (1, 3, 8):
        kinds = {0: (TILE, 15)}
        if n > 2:
            kinds.update({1: (BEGIN, 3), n - 1: (END, 3)})
        ops, at = leaves(n, kinds)
        remote = [relabel(kinds, at, i, n + 1 + j, 2) for j, i in enumerate(sorted(kinds))]
        mine = [relabel(kinds, at, i, 0, 3, own=True) for i in sorted(kinds)]
        acks = [(n + 1 + j, n, 0) + rec[3:] for j, rec in enumerate(mine)]
        docs += [ops + remote, ops + mine, ops + mine + acks[:1], ops + mine + acks]
    eng, o = both(len(docs), ops_per_launch=4)
    apply_both(eng, o, docs)
    for d in range(len(docs)):
        ask_everywhere(eng, o, d, d)
    eng.close()


@pytest.mark.parametrize('n', [64, 65, 128])
def test_wave_boundary_shapes(n):
    """Narrow documents of exactly n leaves with tiles at ordinals 0, 63, 64 and n - 1 (a query's wave covers
    64 leaves).  Three documents each: as built; with the text leaves at the chunk edges removed; with the
    trailing leaf block removed whole too (the last eight leaves: an empty leaf block, its tile found only
    as the leaf a backward search stops on) after a relabelled tile (ordinal 63 where it stays, else 0)."""
    from fluidframework_amd.oplog import REMOVE
    kinds = {i: (TILE, 1 + i % 15) for i in (0, 63, 64, n - 1) if i < n}
    kinds.update({i: (BEGIN if i % 2 else END, 1 << (i % 4)) for i in (5, 6, 61, 66, n - 3)
                  if 0 < i < n - 1 and i not in kinds})
    ops, at = leaves(n, kinds)
    edges = [i for i in (1, 62, 65, n - 2) if 0 < i < n and i not in kinds]
    s, cut = n, []
    for i in sorted(edges, reverse=True):  # (from the right: the positions to the left stay)
        s += 1
        cut.append((s, s - 1, 0, 1 + s % 2, REMOVE, at[i], at[i + 1], None, None, 0))
    # positions once the edge leaves are gone
    after = [p - sum(at[e + 1] - at[e] for e in edges if e < i) for i, p in enumerate(at)]
    tail = [relabel(kinds, after, 63 if 63 < n - 8 else 0, s + 1, 1),
            (s + 2, s + 1, 0, 2, REMOVE, after[n - 8], after[n], None, None, 0)]
    docs = [ops, ops + cut, ops + cut + tail]
    eng, o = both(len(docs), ops_per_launch=16)
    apply_both(eng, o, docs)
    for d in range(len(docs)):
        assert len(eng.state(d)['segs']) == n
        found, deep = ask_everywhere(eng, o, d, (n, d))
        assert found > 100 and deep > 0
    eng.close()
