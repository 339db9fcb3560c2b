"""The findTile / getStackContext checkpoint fixtures (tests/golden/make_tileforms.py): what the CPU and
GPU tests of them share.  A row is one document of a log as the reference's logged client saw it: {log,
doc, name, ids, observer, keys: [tile key, range key], n, promote, counts, checkpoints}; a checkpoint is
{k, len, why, pend, removed, pos, tiles: [reference, [[index, plain], ...]], stacks: [reference, [[index,
plain], ...]]} for each log's first two documents and {..., check} (a digest of the reference's
answers) for the others -- make_tileforms.py documents the fields."""
import hashlib
import json
import os

import numpy as np

from conftest import GOLDEN

LOGS = ['tf_scenarios', 'tf_edit', 'tf_edit_lag', 'tf_edit_reconnect', 'tf_edit_offline', 'tf_wide', 'tf_edit_wide']
CLASS_EDITING, CLASS_LDS, CLASS_C64, CLASS_GROUPS, CLASS_WIDE = 0x40000000, 0x20000000, 0x10000000, 0x08000000, 0x04000000
CLASS_FLAGS = 0xFC000000

_cache = {}


def _read():
    if 'rows' not in _cache:
        with open(os.path.join(GOLDEN, 'tileforms.expected.jsonl')) as f:
            head, *rows = [json.loads(x) for x in f if x.strip()]
        _cache['head'], _cache['rows'] = head, rows
    return _cache['head'], _cache['rows']


def head():
    """The fixture's first row: {counts: {log: {stale_differs, ack_flips, ...}}}."""
    return _read()[0]


def load(name):
    """(batch, rows) of a log, read once."""
    if name not in _cache:
        from fluidframework_amd.oplog import OpBatch
        _cache[name] = (OpBatch.load(os.path.join(GOLDEN, name + '.mtlog')), [r for r in _read()[1] if r['log'] == name])
    return _cache[name]


def span(batch, rows, lo, hi):
    """Records [lo[i], hi[i]) of every row's document as one batch, in the rows' order."""
    from fluidframework_amd.oplog import OpBatch
    idx, rp = [], [0]
    for r, a, b in zip(rows, lo, hi):
        base = int(batch.row_ptr[r['doc']])
        idx.append(np.arange(base + a, base + b))
        rp.append(rp[-1] + b - a)
    return OpBatch(batch.ops[np.concatenate(idx).astype(np.int64)].copy(), batch.payload, np.array(rp, dtype=np.uint32))


def steps(rows):
    """Per step q, per row: its q-th checkpoint, or None once the document is past its last one."""
    n = max(len(r['checkpoints']) for r in rows)
    return [[r['checkpoints'][q] if q < len(r['checkpoints']) else None for r in rows] for q in range(n)]


def label_mask(label):
    """256-bit mask (32 bytes) of the value ids whose label arrays contain L<label>"""
    m = np.zeros(32, dtype=np.uint8)
    for v in range(1, 256):
        if (v >> label) & 1:
            m[v >> 3] |= 1 << (v & 7)
    return m


MASKS = [label_mask(l) for l in range(4)]


def digest(tiles, stacks):
    """A checkpoint's answers as 16 hex digits (make_tileforms.py digest)."""
    return hashlib.sha256(json.dumps([tiles, stacks], separators=(',', ':')).encode()).hexdigest()[:16]


def same_answers(ck, tiles, stacks):
    """Do `tiles` ([position | None, ...]: per position, per label, preceding then not) and `stacks` ([[[marker
    position, refType], ...], ...]: per position, per label) equal the reference's at checkpoint ck?  Exactly:
    the recorded lists, or their digest for a hashed checkpoint.  Returns the indices that differ (hashed:
    [-1])."""
    tiles = [-1 if t is None else t for t in tiles]  # (the fixture's "no tile", as mt_tile_result.pos has it)
    if 'check' in ck:
        return [] if digest(tiles, stacks) == ck['check'] else [-1]
    want_t, want_s = ck['tiles'][0], ck['stacks'][0]
    assert len(tiles) == len(want_t) and len(stacks) == len(want_s)
    return [('tile', i, tiles[i], want_t[i]) for i in range(len(want_t)) if tiles[i] != want_t[i]] + \
        [('stack', i, stacks[i], want_s[i]) for i in range(len(want_s)) if stacks[i] != want_s[i]]


def tile_asks(ck):
    """(position, label, preceding) of a checkpoint's findTile answers, in their recorded order."""
    return [(p, l, prec) for p in ck['pos'] for l in range(4) for prec in (1, 0)]


def stack_asks(ck):
    """(position, label) of a checkpoint's getStackContext answers, in their recorded order."""
    return [(p, l) for p in ck['pos'] for l in range(4)]


def flips(a, b):
    """Queries asked at both checkpoints (of one document, the same local view) whose reference answers
    differ; fully recorded checkpoints only."""
    n = 0
    for ia, p in enumerate(a['pos']):
        if p not in b['pos']:
            continue
        ib = b['pos'].index(p)
        n += sum(a['tiles'][0][8 * ia + j] != b['tiles'][0][8 * ib + j] for j in range(8))
        n += sum(a['stacks'][0][4 * ia + j] != b['stacks'][0][4 * ib + j] for j in range(4))
    return n


def padded(batch, row, lo, hi, b):
    """Records [lo, hi) of the row's document as a one-document batch of exactly b records: b - (hi - lo)
    no-op messages first, which repeat the document's sequence number and minimum sequence number there.  A
    client applies such a message without any change (updateSeqNumbers with nothing to advance), so the
    reference's answers at `hi` stand; the launch that carries the span is b records long."""
    from fluidframework_amd.oplog import OP_DTYPE, OpBatch
    base = int(batch.row_ptr[row['doc']])
    assert 0 <= hi - lo <= b
    done = batch.ops[base:base + lo]
    done = done[done['seq'] > 0]
    cur = int(done['seq'].max()) if len(done) else 0
    msn = int(done['msn'].max()) if len(done) else 0
    pad = np.zeros(b - (hi - lo), dtype=OP_DTYPE)
    pad['seq'], pad['ref_seq'], pad['msn'], pad['client'], pad['type'] = cur, cur, msn, row['ids'][1], 3
    ops = np.concatenate([pad, batch.ops[base + lo:base + hi]])
    return OpBatch(ops, batch.payload, np.array([0, len(ops)], dtype=np.uint32))
