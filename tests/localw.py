"""The wide editing-client fixtures (tests/golden/make_localw.py; include/mtgpu.h "limits"): what the
tests of the wide editing form share.  A row is one document of a log as the reference saw it:
{log, doc, name, ids, n, promote, counts, states: [[k, checksum, segments, flags, [units, digest]], ...][, end]
[, regen][, snapshot]} -- make_localw.py documents the fields."""
import json
import os

import numpy as np

from conftest import GOLDEN

# every log but localw_long (one document of 2100+ records, a test of its own)
LOGS = ['localw_rounds', 'localw_lag', 'localw_promote', 'localw_own_hi', 'localw_reconnect', 'localw_offline']
LONG = 'localw_long'
OP_WIDE = 0x80
CLASS_EDITING, CLASS_GROUPS, CLASS_WIDE = 0x40000000, 0x08000000, 0x04000000
CLASS_FLAGS = 0xFC000000

_cache = {}


def load(name):
    """(batch, rows) of a log, read once."""
    if name not in _cache:
        from fluidframework_amd.oplog import OpBatch
        with open(os.path.join(GOLDEN, name + '.expected.jsonl')) as f:
            rows = [json.loads(x) for x in f if x.strip()]
        _cache[name] = (OpBatch.load(os.path.join(GOLDEN, name + '.mtlog')), rows)
    return _cache[name]


def summary():
    with open(os.path.join(GOLDEN, 'localw.summary.json')) as f:
        return json.load(f)


def events(name):
    with open(os.path.join(GOLDEN, 'localw_events.jsonl')) as f:
        return [r for r in map(json.loads, f) if r['log'] == name]


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
    """The record counts to stop at: per step one count per row -- the q-th checkpoint of every document,
    a document with fewer checkpoints staying at its end."""
    n = max(len(r['states']) for r in rows)
    return [[r['states'][min(q, len(r['states']) - 1)][0] for r in rows] for q in range(n)]


def text_digest(text):
    """(UTF-16 units, digest) of a str, as the fixture keeps getText() (make_localw.py text_digest)."""
    import hashlib
    b = text.encode('utf-16-le', 'surrogatepass')
    return [len(b) // 2, hashlib.sha256(b).hexdigest()[:16]]


def same_state(eng, i, row, k):
    """Is document i of the engine in the reference's state after row's first k records?  Its canonical
    state (MergeEngine.state) hashed by oracle/canon.py and the device's own checksum (mt_checksums) both
    equal the fixture's, the segment count too; the end state in full where the fixture keeps it."""
    from oracle.canon import checksum
    _, want, nseg, _, _ = next(s for s in row['states'] if s[0] == k)
    st = eng.state(i)
    got = ('%016x' % checksum(st), '%016x' % int(eng.checksums()[i]), len(st['segs']))
    assert got == (want, want, nseg), (row['log'], row['doc'], k, got, (want, nseg))
    if k == row['n'] and 'end' in row:
        assert st == row['end'], (row['log'], row['doc'], k)
    return True


def wide_record(batch, i):
    """Does record i need the wide document form (a wide record, or a client id >= 64)?"""
    o = batch.ops[i]
    return bool(int(o['type']) & OP_WIDE) or (int(o['client']) >= 64 and int(o['type']) & 7 != 3)


def pending_edits(batch, row, k):
    """The editing client's edits pending after the document's first k records (logs without reconnects:
    one ack per edit)."""
    a = int(batch.row_ptr[row['doc']])
    ops = batch.ops[a:a + k]
    own = row['ids'][0]
    return int((ops['seq'] == -1).sum()) - int(((ops['seq'] > 0) & (ops['client'] == own)).sum())
