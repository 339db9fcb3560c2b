"""Text reads (include/mtgpu.h "text reads") against the reference's own MergeTreeTextHelper.

tests/golden/textreads.expected.jsonl (make_textreads.py, textreads_ref.js) holds, for the first
documents of seven logs, the getText / getTextAndMarkers calls a seeded plan executed on the reference
at message boundaries, inputs and outputs.  Not on the GPU: fluidframework_amd/textread.py, the read in
plain Python, over the CPU oracle's states at the same boundaries gives every recorded answer.  On the
GPU: the engine follows the same steps -- the batch cut at the plan's record counts -- and
MergeEngine.text_ranges gives them, the "*" placeholder and getTextAndMarkers' cut composed on the host
from the text without placeholders plus the marker list; then edge shapes on small documents, checked
against textread.py on the oracle's state.
"""
import functools
import hashlib
import json
import os
import shutil
import sys

import numpy as np
import pytest

from conftest import GOLDEN

LOGS = ('textreads_spec', 'scenarios', 'markers', 'wide', 'synth_c3', 'local_lag', 'tiles_synth')
TILE_KEY = {'tiles_synth': 0}
FULL_DOCS = 2


@functools.lru_cache(maxsize=None)
def load_fixture():
    with open(os.path.join(GOLDEN, 'textreads.expected.jsonl')) as f:
        lines = [json.loads(x) for x in f if x.strip()]
    by_log = {}
    for r in lines[1:]:
        by_log.setdefault(r['log'], []).append(r)
    return lines[0], by_log


def load_log(name):
    from fluidframework_amd.oplog import OpBatch
    return OpBatch.load(os.path.join(GOLDEN, name + '.mtlog'))


def cut(batch, docs, lo, hi):
    """records [lo[i], hi[i]) of document docs[i], as one batch over the documents in that order"""
    from fluidframework_amd.oplog import OpBatch
    idx, rp = [], [0]
    for d, a, b in zip(docs, lo, hi):
        base = int(batch.row_ptr[d])
        idx.append(np.arange(base + a, base + b))
        rp.append(rp[-1] + b - a)
    idx = np.concatenate(idx) if idx else np.zeros(0, np.int64)
    return OpBatch(batch.ops[idx.astype(np.int64)].copy(), batch.payload, np.array(rp, dtype=np.uint32))


def digest(x):
    return hashlib.sha256(json.dumps(x, separators=(',', ':')).encode()).hexdigest()


def step_cuts(rows):
    """per step s: the record count of every row's document after it (a document out of steps stays)"""
    n_steps = max(len(r['steps']) for r in rows)
    at, out = [0] * len(rows), []
    for s in range(n_steps):
        hi = [r['steps'][s]['k'] if s < len(r['steps']) else at[i] for i, r in enumerate(rows)]
        out.append((list(at), hi))
        at = hi
    return out


@functools.lru_cache(maxsize=None)
def oracle_states(name):
    """[step][row] -> the CPU oracle's canonical state of the row's document at that step (computed once
    per log and shared, never changed)"""
    from oracle import oracle
    oracle.build()
    rows = load_fixture()[1][name]
    batch = load_log(name)
    o = oracle.Oracle(len(rows))
    docs = [r['doc'] for r in rows]
    out = []
    for lo, hi in step_cuts(rows):
        o.apply(cut(batch, docs, lo, hi))
        out.append([o.state(i) for i in range(len(rows))])
    for i in range(len(rows)):
        assert o.error(i)[0] == 0
    return out


def marker_props(seg, tile_key):
    """a marker row's properties as the reference holds them in these logs (js/mtlog.js): key ids as
    "k<id>", the tile key's value id v as the labels ["L<i>" for every bit i of v]"""
    if seg[6] is None:
        return None
    out = {}
    for k, v in seg[6].items():
        if tile_key is not None and k == 'k%d' % tile_key:
            out['referenceTileLabels'] = ['L%d' % i for i in range(8) if (v >> i) & 1]
        else:
            out[k] = v
    return out


def split_props(s):
    """a Marker.toString() as (the text before its properties, the properties parsed)"""
    at = s.find('{')
    return (s, None) if at < 0 else (s[:at], json.loads(s[at:]))


def query_of(op):
    """(start, end, ref_seq | None, client, placeholder unit, want the marker list) of a recorded op;
    the defaults of start / end are the host's: 0 and past the view"""
    from fluidframework_amd.textread import TEXT_END
    view, ph = op[1], op[2] if op[0] == 't' else ''
    star = op[0] == 'm' or ph == '*'
    return (0 if op[3] is None else op[3], TEXT_END if op[4] is None else op[4], None if view is None else view[0],
            0 if view is None else view[1], '' if star else ph, star)


def compose(op, text, markers, segs, tile_key, strings=None):
    """a recorded op's outputs from the device's (or textread's) answer to query_of(op)"""
    from fluidframework_amd.textread import compose_star, has_tile_label, marker_string, split_at_markers
    if op[0] == 'm':
        labelled = [has_tile_label(segs[o][0]['marker'], marker_props(segs[o], tile_key), op[2]) for o, _ in markers]
        texts, ords = split_at_markers(text, markers, labelled)
        return [texts, ords]
    if op[2] != '*':
        return [text]
    # Marker.toString from the state's refType and properties equals the recorded strings, up to the
    # order of the properties (the reference's is their insertion order, which no state keeps)
    assert len(strings) == len(markers), op
    for (o, _), s in zip(markers, strings):
        assert split_props(marker_string(segs[o][0]['marker'], marker_props(segs[o], tile_key))) == split_props(s), (op, s)
    return [compose_star(text, markers, strings)]


def recorded(op, full):
    """(outputs | None, marker strings | None) of an op as the fixture row keeps it"""
    if full:
        return (op[5:6] if op[0] == 't' else op[5:7]), (op[6] if op[0] == 't' and op[2] == '*' else None)
    return None, (op[5] if op[0] == 't' and op[2] == '*' else None)


def test_fixture_shape():
    head, by_log = load_fixture()
    c = head['counts']
    assert set(by_log) == set(LOGS)
    assert c['swap_nonempty'] > 0  # or the plan does not pin String.substring's argument swap
    for key in ('star_markers', 'space_markers', 'tm_cuts', 'tm_absent', 'remote_differs', 'pending'):
        assert c[key] > 0, key
    n = dict.fromkeys(('reads', 'star', 'tm', 'remote', 'swap_nonempty', 'units', 'tm_cuts', 'star_markers'), 0)
    for name, rows in by_log.items():
        batch = load_log(name)
        assert [r['doc'] for r in rows] == list(range(len(rows)))
        for r in rows:
            assert r['err'] is None
            nrec = int(batch.row_ptr[r['doc'] + 1] - batch.row_ptr[r['doc']])
            ks = [s['k'] for s in r['steps']]
            assert ks == sorted(set(ks)) and ks[-1] == nrec, (name, r['doc'], ks, nrec)
            full = r['doc'] < FULL_DOCS
            for s in r['steps']:
                assert ('check' in s) == (not full)
                for op in s['ops']:
                    assert op[0] in ('t', 'm') and (op[1] is None or len(op[1]) == 2)
                    star = op[0] == 't' and op[2] == '*'
                    assert len(op) == (5 + star if not full else 7 if star or op[0] == 'm' else 6), (name, op)
                    n['reads'] += 1
                    n['star'] += star
                    n['tm'] += op[0] == 'm'
                    n['remote'] += op[1] is not None
                    if star:
                        n['star_markers'] += len(op[-1])
                    if full and op[0] == 't':
                        n['units'] += len(op[5].encode('utf-16-le', 'surrogatepass')) // 2
                        n['swap_nonempty'] += op[3] is not None and op[3] > op[4] and op[5] != ''
                    if full and op[0] == 'm':
                        assert len(op[5]) == len(op[6])
                        n['tm_cuts'] += len(op[6])
    for key in ('reads', 'star', 'tm', 'remote', 'star_markers'):
        assert n[key] == c[key], key
    # the fully recorded documents alone pin the swap; they hold part of the counted units and cuts
    assert 0 < n['swap_nonempty'] <= c['swap_nonempty'] and 0 < n['units'] <= c['units'] and 0 < n['tm_cuts'] <= c['tm_cuts']


@pytest.mark.parametrize('name', LOGS)
def test_python_read_reproduces_the_reference(name):
    """textread.get_text (with compose_star / split_at_markers) over the oracle's states gives every
    recorded answer: exactly on the fully recorded documents, by digest on the others."""
    from fluidframework_amd.textread import get_text
    rows = load_fixture()[1][name]
    states = oracle_states(name)
    checked = 0
    for i, r in enumerate(rows):
        full = r['doc'] < FULL_DOCS
        for s, st in enumerate(r['steps']):
            segs = states[s][i]['segs']
            outs = []
            for op in st['ops']:
                start, end, ref_seq, client, ph, _ = query_of(op)
                text, markers = get_text(segs, start, end, ref_seq, client, ph)
                want, strings = recorded(op, full)
                got = compose(op, text, markers, segs, TILE_KEY.get(name), strings)
                outs.append(got)
                if full:
                    assert got == want, (name, r['doc'], st['k'], op[:5], got)
                checked += 1
            if not full:
                assert digest(outs) == st['check'], (name, r['doc'], st['k'])
    assert checked > 100


def test_python_read_rules():
    from fluidframework_amd.textread import compose_star, get_length, get_text, marker_string, split_at_markers
    T = lambda t, seq=1, cl=1, rseq=-1, rcl=-1, ovl=(): [t, seq, cl, rseq, rcl, list(ovl), None]
    segs = [T('abc'), T({'marker': 1}), T('defgh', seq=5, cl=2), T('xy', rseq=7, rcl=2), T('Z', seq=-1, cl=3)]
    assert get_text(segs)[0] == 'abcdefghZ' and get_length(segs) == 10
    assert get_text(segs, placeholder=' ') == ('abc defghZ', [(1, 3)])
    assert get_text(segs, 5, 8) == ('efg', []) and get_text(segs, 7, 5)[0] == 'ef'  # substring's swap
    assert get_text(segs, 8, 2)[0] == '' and get_text(segs, -3, 2)[0] == 'ab' and get_text(segs, 0, 0)[0] == ''
    assert get_text(segs, 3, 4, placeholder='#') == ('#', [(1, 0)]) and get_text(segs, 4, 3, placeholder='#')[0] == ''
    # client 1 at refSeq 4: not yet the insert at 5, still the text removed at 7; the pending insert is its author's alone
    assert get_text(segs, ref_seq=4, client=1)[0] == 'abcxy' and get_text(segs, ref_seq=9, client=3)[0] == 'abcdefghZ'
    assert get_text(segs, ref_seq=6, client=2)[0] == 'abcdefgh'
    assert marker_string(1) == 'M Tile:  ' and marker_string(6, {}) == 'M RangeBegin; RangeEnd:  {}'
    assert marker_string(1, {'referenceTileLabels': ['a', 'b'], 'markerId': 'm1'}) == \
        'M Tile (m1) : tile -- a; b {"referenceTileLabels":["a","b"],"markerId":"m1"}'
    assert marker_string(2, {'referenceTileLabels': ['a']}) == 'M RangeBegin:  {"referenceTileLabels":["a"]}'  # no Tile
    assert marker_string(4, {'referenceRangeLabels': ['r']}) == 'M RangeEnd: range end -- r {"referenceRangeLabels":["r"]}'
    assert compose_star('abcd', [(1, 1), (2, 1), (5, 4)], ['X', 'Y', 'Z']) == 'a\nX\nYbcd\nZ'
    assert split_at_markers('abcdef', [(1, 2), (3, 2), (4, 5)], [True, False, True]) == (['ab', 'cde'], [1, 4])


HAVE_REF = os.path.isdir('/root/reference/packages/dds/merge-tree/src') and shutil.which('node')


@pytest.mark.reference
@pytest.mark.skipif(not HAVE_REF, reason='reference sources / node not present (GPU box)')
def test_fixture_regenerates_byte_identically():
    sys.path.insert(0, GOLDEN)
    import make_textreads
    text, spec, _ = make_textreads.generate()
    with open(os.path.join(GOLDEN, 'textreads.expected.jsonl')) as f:
        assert f.read() == text
    kept = load_log('textreads_spec')
    assert np.array_equal(kept.ops, spec.ops) and np.array_equal(kept.payload, spec.payload) and \
        np.array_equal(kept.row_ptr, spec.row_ptr)


# ---- on the GPU ------------------------------------------------------------------------------------

def engine_read(eng, reads):
    """reads: [(doc, start, end, ref_seq | None, client, placeholder, want markers)] -> (texts, markers)"""
    from fluidframework_amd.textread import TEXT_LOCAL, TEXT_MARKERS
    q = eng.text_queries([r[0] for r in reads], [r[1] for r in reads], [r[2] for r in reads],
                         [TEXT_LOCAL if r[3] is None else r[3] for r in reads], [r[4] for r in reads],
                         [r[5] for r in reads], [TEXT_MARKERS if r[6] else 0 for r in reads])
    return eng.text_ranges(q)


@pytest.mark.gpu
@pytest.mark.parametrize('b', [1, 7, 32])
@pytest.mark.parametrize('name', LOGS)
def test_engine_text_reads_match_reference(name, b):
    """Every recorded read through text_ranges, all documents' reads of a step in one call; no document
    errs.  At each step text_lengths of the whole local view (with a placeholder: getLength) equals
    get_length, and mt_get_text equals text_ranges of the whole local view without placeholder."""
    from fluidframework_amd.engine import MergeEngine
    from fluidframework_amd.textread import TEXT_END
    rows = load_fixture()[1][name]
    batch = load_log(name)
    states = oracle_states(name)
    docs = [r['doc'] for r in rows]
    eng = MergeEngine(len(rows), ops_per_launch=b)
    for s, (lo, hi) in enumerate(step_cuts(rows)):
        eng.apply(cut(batch, docs, lo, hi))
        on = [i for i, r in enumerate(rows) if s < len(r['steps'])]
        reads = [(i,) + query_of(op) for i in on for op in rows[i]['steps'][s]['ops']]
        texts, markers = engine_read(eng, reads)
        j = 0
        for i in on:
            st, full = rows[i]['steps'][s], rows[i]['doc'] < FULL_DOCS
            segs = states[s][i]['segs']
            outs = []
            for op in st['ops']:
                want, strings = recorded(op, full)
                got = compose(op, texts[j], markers[j], segs, TILE_KEY.get(name), strings)
                outs.append(got)
                if full:
                    assert got == want, (name, rows[i]['doc'], b, st['k'], op[:5], got)
                j += 1
            if not full:
                assert digest(outs) == st['check'], (name, rows[i]['doc'], b, st['k'])
        assert j == len(reads)
        whole = eng.text_lengths(eng.text_queries(on, 0, TEXT_END, placeholders=' '))
        assert [int(x) for x in whole['units']] == [eng.length(i) for i in on]
        plain, _ = eng.text_ranges(eng.text_queries(on))
        assert plain == [eng.text(i) for i in on]
    for i, r in enumerate(rows):
        assert eng.error(i) == (0, 0), (name, r['doc'], eng.error(i))
    eng.close()


def build_batch(docs):
    """docs: per document [(seq, ref, msn, client, type, flags, pos1, pos2, text)] -> OpBatch; a text with
    a unit above U+00FF makes a wide record"""
    from fluidframework_amd.oplog import OP_DTYPE, OP_WIDE, OpBatch, encode_text
    rows, payload, rp = [], bytearray(), [0]
    for ops in docs:
        for seq, ref, msn, client, typ, flags, p1, p2, text in ops:
            b, wide = encode_text(text)
            rows.append((seq, ref, msn, client, typ | (OP_WIDE if wide else 0), flags, p1, p2, len(payload), len(b)))
            payload += b
        rp.append(len(rows))
    return OpBatch(np.array(rows, dtype=OP_DTYPE) if rows else np.zeros(0, OP_DTYPE),
                   np.frombuffer(bytes(payload), dtype=np.uint8), np.array(rp, dtype=np.uint32))


def leaves_doc(n, marker_at=(), wide=False):
    """n leaves of 1-3 units by alternating clients at msn 0 (none is appended to its neighbour); the
    leaves in marker_at are Tile markers"""
    from fluidframework_amd.oplog import F_MARKER, INSERT
    ops, pos = [], 0
    for i in range(n):
        if i in marker_at:
            ops.append((i + 1, i, 0, 1 + i % 2, INSERT, F_MARKER, pos, 0, '\x01'))
            pos += 1
        else:
            t = ''.join(chr((0x3b1 if wide else 97) + (i + j) % 24) for j in range(1 + i % 3))
            ops.append((i + 1, i, 0, 1 + i % 2, INSERT, 0, pos, 0, t))
            pos += len(t)
    return ops


def both(docs, **kw):
    """(engine, the oracle's segs per document) after the same batch"""
    from fluidframework_amd.engine import MergeEngine
    from oracle import oracle
    oracle.build()
    batch = build_batch(docs)
    eng = MergeEngine(len(docs), ops_per_launch=32, **kw)
    eng.apply(batch)
    o = oracle.Oracle(len(docs)).apply(batch)
    for d in range(len(docs)):
        assert eng.error(d) == (0, 0) and o.error(d)[0] == 0, d
    return eng, [o.state(d)['segs'] for d in range(len(docs))]


def check_reads(eng, segs, reads):
    from fluidframework_amd.textread import get_text
    texts, markers = engine_read(eng, reads)
    for r, t, m in zip(reads, texts, markers):
        wt, wm = get_text(segs[r[0]], r[1], r[2], r[3], r[4], r[5])
        assert t == wt and m == (wm if r[6] else []), (r, t, wt, m, wm)
    return texts, markers


def boundaries(segs):
    """the local view's position of every leaf boundary"""
    from fluidframework_amd.textread import view_len
    out, p = [0], 0
    for s in segs:
        p += view_len(s, None, 0)
        out.append(p)
    return out


@pytest.mark.gpu
def test_chunk_boundary_shapes():
    """Documents of 0, 63, 64, 65 and 129 leaves of 1-3 units, a wide one and narrow ones in one batch:
    read whole, and with start / end on every leaf boundary around leaves 64 and 128 (start > end
    included); markers as leaves 63 and 64 with a placeholder and with the marker list; zero queries."""
    from fluidframework_amd.textread import TEXT_END
    sizes = [0, 63, 64, 65, 129, 129, 66]
    docs = [leaves_doc(n) for n in sizes[:5]] + [leaves_doc(129, wide=True), leaves_doc(66, marker_at=(63, 64))]
    eng, segs = both(docs)
    assert [len(s) for s in segs] == sizes and eng.seg_counts().tolist() == sizes
    reads, first = [], []
    for d, n in enumerate(sizes):
        bd = boundaries(segs[d])
        first.append(len(reads))
        reads += [(d, 0, TEXT_END, None, 0, '', False), (d, 0, TEXT_END, None, 0, '#', True), (d, -5, bd[-1] + 9, None, 0, '', True)]
        near = sorted({i for c in (64, 128) for i in range(c - 2, c + 3) if 0 <= i <= n})
        for i in near:
            for j in near:
                reads.append((d, bd[i], bd[j], None, 0, '#' if (i + j) % 2 else '', (i + j) % 3 == 0))
            reads += [(d, bd[i], TEXT_END, None, 0, '', False), (d, 0, bd[i], None, 0, '', False),
                      (d, bd[i] + 1, bd[i] - 1, None, 0, '', False), (d, bd[i] - 1, bd[i] + 1, None, 0, '#', True)]
    texts, markers = check_reads(eng, segs, reads)
    assert texts[0] == '' and any(ord(c) > 0xFF for c in texts[first[5]]) and len(texts[first[4]]) > 200
    assert markers[first[6] + 1] == [(63, boundaries(segs[6])[63]), (64, boundaries(segs[6])[63] + 1)]
    assert eng.text_ranges(eng.text_queries([])) == ([], []) and len(eng.text_lengths(eng.text_queries([]))) == 0
    eng.close()


@pytest.mark.gpu
def test_long_segment_removed_edges_and_views():
    """One 200-unit segment read at [3, 150) (more than two output strides from one source segment) and
    with start > end inside it; removed leaves at the chunk edges; an observer document read in a
    (refSeq, client) view that hides a later insert and still shows a later remove's text; an editing
    document with a pending insert and a pending removal inside the range (local view)."""
    from fluidframework_amd.oplog import INSERT, REMOVE
    from fluidframework_amd.textread import TEXT_END, get_text
    long = ''.join(chr(65 + i % 26) for i in range(200))
    d0 = [(1, 0, 0, 1, INSERT, 0, 0, 0, 'ab'), (2, 1, 0, 2, INSERT, 0, 2, 0, long), (3, 2, 0, 1, INSERT, 0, 202, 0, 'yz')]
    d1 = leaves_doc(131)
    bd = boundaries([[op[8], 0, 0, -1, -1, [], None] for op in d1])
    n = len(d1)  # leaves 62..65 and 127..128 removed: a chunk's last and next first leaves hidden
    d1 += [(n + 1, n, 0, 1, REMOVE, 0, bd[62], bd[66], ''), (n + 2, n + 1, 0, 2, REMOVE, 0, bd[127] - (bd[66] - bd[62]), bd[129] - (bd[66] - bd[62]), '')]
    d2 = [(1, 0, 0, 1, INSERT, 0, 0, 0, 'hello world'), (2, 1, 0, 2, INSERT, 0, 5, 0, ' big'), (3, 1, 0, 1, REMOVE, 0, 0, 3, ''),
          (4, 3, 0, 2, INSERT, 0, 0, 0, '>>')]
    # client 1 edits: a pending insert and a pending removal, after two sequenced messages
    d3 = [(1, 0, 0, 2, INSERT, 0, 0, 0, 'remote text'), (2, 1, 0, 3, INSERT, 0, 6, 0, ' more'),
          (-1, 0, 0, 1, INSERT, 0, 3, 0, 'LOCAL'), (-1, 0, 0, 1, REMOVE, 0, 10, 14, '')]
    eng, segs = both([d0, d1, d2, d3])
    assert sum(1 for s in segs[1] if s[3] != -1) >= 6
    assert any(s[1] == -1 for s in segs[3]) and any(s[3] == -1 and s[4] != -1 for s in segs[3])
    reads = [(0, 3, 150, None, 0, '', False), (0, 150, 3, None, 0, '', False), (0, 201, 3, None, 0, '', False),
             (0, 0, TEXT_END, None, 0, '', False), (0, 100, 101, None, 0, '', False)]
    b1 = boundaries(segs[1])
    reads += [(1, 0, TEXT_END, None, 0, '', False)] + [(1, b1[i], b1[j], None, 0, '', False)
                                                       for i in (60, 62, 64, 66, 126, 128, 130) for j in (61, 63, 67, 127, 129, 131)]
    # document 2 as client 1 saw it at refSeq 1 (before ' big' at 2, 'hel' still there: its own later
    # remove hides it for itself only at its seq), as client 2 at refSeq 1, and at the ends of the window
    reads += [(2, 0, TEXT_END, rs, c, '', False) for rs in (0, 1, 2, 3, 4) for c in (1, 2, 3)]
    reads += [(2, 2, 9, 1, 3, '', False), (2, 9, 2, 2, 3, '', False)]
    reads += [(3, 0, TEXT_END, None, 0, '', False), (3, 2, 16, None, 0, '', False), (3, 12, 4, None, 0, '', False)]
    texts, _ = check_reads(eng, segs, reads)
    assert texts[0] == ('ab' + long)[3:150] and texts[1] == texts[0] and len(texts[0]) == 147 and texts[2] == long[1:199]
    assert get_text(segs[2], ref_seq=1, client=3)[0] == 'hello world' and get_text(segs[2], ref_seq=2, client=3)[0] == 'hello big world'
    assert get_text(segs[2], ref_seq=2, client=1)[0] == 'lo big world'
    assert 'LOCAL' in texts[-3] and len(texts[-3]) == len('remote text more') + 5 - 4
    eng.close()


@pytest.mark.gpu
def test_row_capacity_and_bad_queries_on_the_device():
    """The device variant with rows of a capacity the caller chose, smaller than the answer: the whole
    count is reported and nothing is written past the row; a document id past the engine's documents
    gets MT_TEXT_BAD_QUERY and the queries around it their answers."""
    from fluidframework_amd.hipmem import DeviceBuffer
    from fluidframework_amd.textread import (TEXT_BAD_QUERY, TEXT_COUNT_DTYPE, TEXT_END, TEXT_MARKER_DTYPE, TEXT_MARKERS,
                                             get_text)
    eng, segs = both([leaves_doc(70, marker_at=(3, 63, 64, 69)), leaves_doc(5)])
    q = eng.text_queries([0, 2, 1 << 30, 1, 0], 0, TEXT_END, placeholders=['#', '', '', '', ''], flags=TEXT_MARKERS)
    want = [get_text(segs[d], placeholder=p) for d, p in ((0, '#'), (1, ''), (0, ''))]
    caps, mcaps = [10, 4, 4, 3, 1000], [2, 1, 1, 1, 8]
    rp = np.concatenate([[0], np.cumsum(caps)]).astype(np.uint32)
    mrp = np.concatenate([[0], np.cumsum(mcaps)]).astype(np.uint32)
    fill = np.full(int(rp[-1]), 0xEEEE, dtype='<u2')
    mfill = np.zeros(int(mrp[-1]), dtype=TEXT_MARKER_DTYPE)
    mfill['ordinal'] = -7
    dq, drp, dmrp = DeviceBuffer(q.nbytes).upload(q), DeviceBuffer(rp.nbytes).upload(rp), DeviceBuffer(mrp.nbytes).upload(mrp)
    du, dm = DeviceBuffer(fill.nbytes).upload(fill), DeviceBuffer(mfill.nbytes).upload(mfill)
    dc = DeviceBuffer(len(q) * TEXT_COUNT_DTYPE.itemsize)
    eng.text_ranges_device(dq.ptr, len(q), 0, 0, 0, 0, dc.ptr)  # the count pass
    counts = dc.download(TEXT_COUNT_DTYPE)
    assert counts['units'].tolist() == [len(want[0][0]), TEXT_BAD_QUERY, TEXT_BAD_QUERY, len(want[1][0]), len(want[2][0])]
    assert counts['markers'].tolist() == [4, 0, 0, 0, 4]
    eng.text_ranges_device(dq.ptr, len(q), drp.ptr, du.ptr, dmrp.ptr, dm.ptr, dc.ptr)
    assert np.array_equal(dc.download(TEXT_COUNT_DTYPE), counts)
    u, m = du.download('<u2'), dm.download(TEXT_MARKER_DTYPE)
    row = lambda k: u[rp[k]:rp[k + 1]].tobytes().decode('utf-16-le')
    assert row(0) == want[0][0][:10] and row(3) == want[1][0][:3] and row(4)[:len(want[2][0])] == want[2][0]
    assert (u[rp[1]:rp[3]] == 0xEEEE).all() and (u[int(rp[4]) + len(want[2][0]):] == 0xEEEE).all()
    assert [(int(x['ordinal']), int(x['out_offset'])) for x in m[0:2]] == want[0][1][:2]
    assert [(int(x['ordinal']), int(x['out_offset'])) for x in m[mrp[4]:mrp[4] + 4]] == want[2][1]
    assert (m['ordinal'][2:5] == -7).all() and (m['ordinal'][int(mrp[4]) + 4:] == -7).all()
    # the host entry refuses what it can check
    from fluidframework_amd.engine import MtError
    with pytest.raises(MtError, match='bad argument'):
        eng.text_ranges(eng.text_queries([2]))
    eng.close()


@pytest.mark.gpu
def test_workspace_class_document():
    """A document past 2048 segments (a workspace class), read whole and across several chunks."""
    from fluidframework_amd.textread import TEXT_END
    eng, segs = both([leaves_doc(2300)], seg_capacity=4096)
    assert len(segs[0]) == 2300
    bd = boundaries(segs[0])
    reads = [(0, 0, TEXT_END, None, 0, '', False), (0, bd[1000] + 1, bd[1300] - 1, None, 0, '', False),
             (0, bd[2047], bd[2049], None, 0, '', False), (0, bd[2299], bd[2300] + 5, None, 0, '', False),
             (0, bd[2300], bd[2300] + 5, None, 0, '', False)]
    texts, _ = check_reads(eng, segs, reads)
    assert len(texts[0]) == bd[-1] and texts[4] == ''
    eng.close()


@pytest.mark.gpu
def test_documents_with_a_sticky_error_answer_from_their_last_good_state():
    """tests/golden/errors.*: logs on which the reference's applyMsg throws.  A halted document's reads
    come from its state before the failing message, the same state mt_get_text / mt_get_length read."""
    from conftest import load_golden
    from fluidframework_amd.engine import MergeEngine
    from fluidframework_amd.textread import TEXT_END, get_text
    batch, exp = load_golden('errors')
    eng = MergeEngine(batch.n_docs, ops_per_launch=32)
    eng.apply(batch)
    docs = list(range(batch.n_docs))
    assert any(eng.error(d)[0] != 0 for d in docs)
    texts, _ = eng.text_ranges(eng.text_queries(docs))
    assert texts == [eng.text(d) for d in docs]
    assert [int(x) for x in eng.text_lengths(eng.text_queries(docs, 0, TEXT_END, placeholders=' '))['units']] == \
        [eng.length(d) for d in docs]
    for d in docs:
        assert texts[d] == get_text(eng.state(d)['segs'])[0], d
    eng.close()
