#!/usr/bin/env python3
"""Wide editing-client fixtures FROM THE REFERENCE ITSELF (build container only; needs node and the
reference's transpile under oracle/_tsref).

tests/golden/localw_ref.js runs a farm of four reference Clients behind a toy sequencer and logs what
the editing client sees (the pattern of oracle/tsref/local_farm.js) with content past the narrow
limits of include/mtgpu.h: UTF-16 text (Latin-1, BMP CJK, surrogate pairs), keys 0..31, value ids up
to 65535, markers with an id of their own (value ids from 256), client ids >= 64 and >= 256.

  localw_rounds     every client catches up each round               6 documents, no run dropped
  localw_lag        the editing client lags                           6
  localw_promote    narrow at first; turns wide with edits pending: its own wide local edit (documents
                    0, 1), a remote wide op (2, 3), a remote client id >= 64 (4, 5); a checkpoint on
                    each side of the promoting record (`promote`: {k, route, pending})
  localw_own_hi     the editing client's own id is 70, 90, 300 (documents 0, 1, 2)
  localw_reconnect  the reconnect farm, the regenerated ops in `regen`     4
  localw_offline    the editing client goes offline: more than 64 edits pending at once   2
  localw_long       one document of 2100+ records that stays under 900 segments

<log>.mtlog: the records.  <log>.expected.jsonl: one row per document {log, doc, name, ids, n, promote,
counts, states: [[k, checksum, segments, flags, [units, digest]], ...][, end][, regen][, snapshot: [k,
SnapshotV1 entries]]}, kept small as refinsert.expected.jsonl is: a state (the form of
oracle/tsref/replay_ref.js, after k records, the last one the end) is its canonical checksum
(oracle/canon.py, what mt_checksums computes: segments, tree, seq and msn), its segment count and the
flags 'w' (a wide insert pending: non-Latin-1 text, a key >= 8 or a value id > 255) and 'r' (a removal
pending); the editing client's getText() there is its UTF-16 units and text_digest of them.  `end` is the
end state in full, for each log's first document where it has at most FULL_STATE_SEGS segments.
`snapshot` (localw_lag's first document): the reference's SnapshotV1 at the first checkpoint with a wide
insert pending.  localw_events.jsonl: the editing client's callbacks per document as count + SHA-256, in
full for each log's first document (where small).  localw.summary.json: runs tried / kept / dropped per log and the farm's own counts.
Fixtures are data only (inputs and reference outputs).
"""
import hashlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

# (log, kind, seed, documents, edits over all clients)
LOGS = (('localw_rounds', 'rounds', 101, 6, 300), ('localw_lag', 'lag', 102, 6, 300),
        ('localw_promote', 'promote', 103, 6, 240), ('localw_own_hi', 'own_hi', 104, 3, 300),
        ('localw_reconnect', 'reconnect', 105, 4, 260), ('localw_offline', 'offline', 106, 2, 420),
        ('localw_long', 'long', 107, 1, 2150))
FULL_EVENTS_BYTES = 30_000
FULL_STATE_SEGS = 120


def text_digest(text):
    """A str's UTF-16 code units (lone surrogates kept) as 16 hex digits."""
    return hashlib.sha256(text.encode('utf-16-le', 'surrogatepass')).hexdigest()[:16]


def wide_pending(seg):
    props = seg[6] or {}
    return seg[1] == -1 and ((isinstance(seg[0], str) and any(ord(c) > 255 for c in seg[0])) or
                             any(int(k[1:]) >= 8 or (v or 0) > 255 for k, v in props.items()))


def compact_state(k, state, text):
    from oracle.canon import checksum
    flags = ('w' if any(wide_pending(s) for s in state['segs']) else '') + \
            ('r' if any(s[3] == -1 and s[4] != -1 for s in state['segs']) else '')
    units = len(text.encode('utf-16-le', 'surrogatepass')) // 2
    return [k, '%016x' % checksum(state), len(state['segs']), flags, [units, text_digest(text)]]


def tuples(records):
    return [(s, r, m, c, t, p1, p2, text, None if props is None else {int(k): v for k, v in props.items()}, flags)
            for (s, r, m, c, t, p1, p2, text, props, flags) in records]


def dumps(x):
    return json.dumps(x, separators=(',', ':'))


def main(outdir=HERE):
    from fluidframework_amd.oplog import build_batch
    summary, ev_rows = {}, []
    for log, kind, seed, n_docs, edits in LOGS:
        res = subprocess.run(['node', os.path.join(HERE, 'localw_ref.js'), kind, str(seed), str(n_docs), str(edits)],
                             check=True, capture_output=True, text=True)
        *docs, tail = [json.loads(x) for x in res.stdout.strip().split('\n')]
        assert tail['kept'] == n_docs, (log, tail)
        if log == 'localw_rounds':
            assert tail['dropped'] == 0, tail
        counts = {}
        for d in docs:
            for k, v in d['counts'].items():
                counts[k] = max(counts.get(k, 0), v) if k == 'pendingMax' else counts.get(k, 0) + v
        summary[log] = dict(tail, counts=counts, records=[len(d['records']) for d in docs], segs=[d['segs'] for d in docs])
        build_batch([tuples(d['records']) for d in docs]).save(os.path.join(outdir, log + '.mtlog'))
        with open(os.path.join(outdir, log + '.expected.jsonl'), 'w') as f:
            for i, d in enumerate(docs):
                row = dict(log=log, doc=i, name=d['name'], ids=d['ids'], n=len(d['records']), promote=d['promote'],
                           counts=d['counts'], states=[compact_state(*s[:3]) for s in d['states']])
                end = d['states'][-1][1]
                assert not any(s[1] == -1 or (s[3] == -1 and s[4] != -1) for s in end['segs']), (log, i)
                if i == 0 and len(end['segs']) <= FULL_STATE_SEGS:
                    row['end'] = end
                if d['regen']:
                    row['regen'] = d['regen']
                snap = next(([s[0], s[3]] for s, c in zip(d['states'], row['states']) if len(s) > 3 and 'w' in c[3]), None)
                if snap:
                    row['snapshot'] = snap
                f.write(dumps(row) + '\n')
            for i, d in enumerate(docs):
                ev = d['events']
                body = dumps(ev)
                rec = dict(log=log, doc=i, n=len(ev), sha256=hashlib.sha256(body.encode()).hexdigest())
                if i == 0 and len(body) <= FULL_EVENTS_BYTES:
                    rec['events'] = ev
                ev_rows.append(dumps(rec))
        print(log, 'tried', tail['tried'], 'kept', tail['kept'], 'dropped', tail['dropped'],
              sum(len(d['records']) for d in docs), 'records')
    with open(os.path.join(outdir, 'localw_events.jsonl'), 'w') as f:
        f.write('\n'.join(ev_rows) + '\n')
    with open(os.path.join(outdir, 'localw.summary.json'), 'w') as f:
        f.write(json.dumps(summary, indent=1, sort_keys=True) + '\n')
    print(dumps({k: (v['tried'], v['kept'], v['dropped']) for k, v in summary.items()}))


if __name__ == '__main__':
    main(*sys.argv[1:2])
