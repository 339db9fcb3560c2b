#!/usr/bin/env python3
"""Marker-relative op fixtures FROM THE REFERENCE ITSELF (build container only; needs the reference and
node).

tests/golden/relpos_ref.js runs a farm of reference Clients (the transpile of oracle/tsref/build_ref.py)
whose clients insert text and markers with ids, remove ranges and annotate markers through
Client.annotateMarker -- the op with relativePos1 / relativePos2 that every receiver resolves against
its own tree -- and logs the stream as an observer sees it and as the editing client c1 sees it (its own
annotateMarker as the absolute local edit its host resolves, its ack in the relative form).  A few
hand-written ops from a sender that is no Client add the forms annotateMarker never produces: an
unknown id, offsets on both sides, a relative REMOVE, a relative INSERT, a GROUP with a relative member.

  relpos.mtlog       the observers' logs          relpos_c1.mtlog   the same runs as c1 sees them
  relpos_wide.mtlog  observers' logs of a wide variant: UTF-16 text, marker ids whose value ids pass
                     255, the "markerId" key interned as key 9, clients 70 and 99
  relpos.expected.jsonl  first row: the counts; then one row per (log, doc):
      {log, doc, n, checkpoints: [{k, checksum, named[, state]}], rel, events: {n, sha256}, pfr}
    (relpos_ref.js documents the fields).  The reference's outputs are kept small as textreads.expected.jsonl
    keeps them: every checkpoint state as its canonical checksum (oracle/canon.py, what mt_checksums
    computes) and as `named`, the SHA-256 of the state with long client ids and properties by name (what a
    host that interns in its own order can reproduce); in full for document 0's middle and last checkpoints.
    The callbacks as their count and the SHA-256 of the canonical list.

In the records a marker id "m<n>" is value id n of the log's markerId key (MARKER_KEY below); mtlog.js
reads them back with {markerKey}.  Fixtures are data only (inputs and reference outputs).
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

MARKER_KEY = {'relpos': 3, 'relpos_c1': 3, 'relpos_wide': 9}


def extras(unknown, text):
    """The hand-written ops (relpos_ref.js `extra`): [round, op[, minPos, pick]]."""
    any_ = '$any'
    rows = [
        (4, {'type': 2, 'relativePos1': {'id': unknown, 'before': True}, 'relativePos2': {'id': unknown}, 'props': {'k1': 2}}),
        (7, {'type': 2, 'relativePos1': {'id': any_, 'before': True, 'offset': 2}, 'relativePos2': {'id': any_, 'offset': 3},
             'props': {'k2': 3}}, 3, 1),
        (10, {'type': 1, 'relativePos1': {'id': any_, 'before': True}, 'relativePos2': {'id': any_, 'offset': 2}}, 0, 2),
        (13, {'type': 0, 'relativePos1': {'id': any_}, 'seg': text}, 0, 3),
        (16, {'type': 3, 'ops': [{'type': 0, 'pos1': 0, 'seg': 'G'},
                                 {'type': 2, 'relativePos1': {'id': any_, 'before': True}, 'relativePos2': {'id': any_},
                                  'props': {'k0': 4}},
                                 {'type': 1, 'pos1': 0, 'pos2': 1}]}, 0, 4),
        (22, {'type': 1, 'relativePos1': {'id': any_, 'before': True}, 'relativePos2': {'id': any_}}, 0, 5),
        (28, {'type': 0, 'relativePos1': {'id': any_, 'before': True, 'offset': 1}, 'seg': {'text': text, 'props': {'k1': 1}}}, 2, 6),
        (34, {'type': 1, 'relativePos1': {'id': unknown, 'before': True}, 'relativePos2': {'id': unknown}}),
        (40, {'type': 2, 'relativePos1': {'id': any_, 'before': True}, 'relativePos2': {'id': any_},
              'props': {'k0': None, 'k2': 1, 'markerId': '$id'}, 'combiningOp': {'name': 'rewrite'}}, 0, 7),
    ]
    return [dict(round=r[0], op=r[1], minPos=(r[2] if len(r) > 2 else 0), pick=(r[3] if len(r) > 3 else 0)) for r in rows]


SETS = (
    dict(name='relpos', docs=4, seed=31, ops=700, clients=[1, 2, 3, 4], markerKey=3, firstId=1, unknownId=250, wide=False,
         views=['observer', 'c1'], every=120, phantom=9, extra=extras('m250', 'REL')),
    dict(name='relpos_wide', docs=2, seed=32, ops=700, clients=[1, 2, 70, 3], markerKey=9, firstId=230, unknownId=60000,
         wide=True, views=['observer'], every=150, phantom=99, extra=extras('m60000', 'ρελ')),
)
# what every log set must hold at least once (the header row's counts)
NEED = ('live', 'tomb', 'split', 'none', 'ord64', 'ord128', 'insert_rel', 'remove_rel', 'group_rel', 'offsets', 'pfr',
        'pfr_remote', 'pfr_differs')
NEED_C1 = ('pend_before', 'pend_after')


def digest(value):
    """SHA-256 of a JSON value in one fixed serialisation."""
    return hashlib.sha256(json.dumps(value, separators=(',', ':'), sort_keys=True).encode()).hexdigest()


def by_name(state, mk):
    """A canonical state as a host reports it that interns clients, keys and values in its own order
    (BatchClient.getState): long client ids, properties by name, overlap sets sorted."""
    def cid(c):
        return c if c < 0 else 'c%d' % c
    segs = []
    for text, seq, client, rseq, rclient, ov, props in state['segs']:
        if props is not None:
            props = {('markerId' if k == 'k%d' % mk else k): ('m%d' % v if k == 'k%d' % mk and v is not None else v)
                     for k, v in props.items()}
        segs.append([text, seq, cid(client), rseq, cid(rclient), sorted(cid(o) for o in ov), props])
    return dict(state, segs=segs)


def compact(checkpoints, mk, full):
    """[{k, checksum, named[, state]}] of the driver's [{k, state}]."""
    from oracle.canon import checksum
    keep = {len(checkpoints) // 2, len(checkpoints) - 1} if full else set()
    out = []
    for i, c in enumerate(checkpoints):
        row = dict(k=c['k'], checksum='%016x' % checksum(c['state']), named=digest(by_name(c['state'], mk)))
        if i in keep:
            row['state'] = c['state']
        out.append(row)
    return out


def tuples(records):
    return [(s, r, m, c, t, p1, p2, text, None if props is None else {int(k): v for k, v in props.items()}, flags, r1, r2)
            for (s, r, m, c, t, p1, p2, text, props, flags, r1, r2) in records]


def main(outdir=HERE):
    from fluidframework_amd.oplog import build_batch
    driver = os.path.join(HERE, 'relpos_ref.js')
    rows, header = [], {}
    for cfg in SETS:
        with tempfile.NamedTemporaryFile('w', suffix='.json', delete=False) as f:
            json.dump({k: v for k, v in cfg.items() if k != 'name'}, f)
        try:
            res = subprocess.run(['node', driver, f.name], check=True, capture_output=True, text=True)
        finally:
            os.unlink(f.name)
        docs = [json.loads(x) for x in res.stdout.strip().split('\n')]
        counts = {}
        for d in docs:
            for k, v in d['counts'].items():
                counts[k] = counts.get(k, 0) + v
        assert counts['skipped'] == 0, '%s: %d relative ops skipped' % (cfg['name'], counts['skipped'])
        for k in NEED + (NEED_C1 if 'c1' in cfg['views'] else ()):
            assert counts[k] > 0, '%s: no case of %s' % (cfg['name'], k)
        header[cfg['name']] = counts
        for view, name in (('observer', cfg['name']), ('c1', cfg['name'] + '_c1')):
            if view not in cfg['views']:
                continue
            build_batch([tuples(d[view]['records']) for d in docs]).save(os.path.join(outdir, name + '.mtlog'))
            for i, d in enumerate(docs):
                v = d[view]
                rows.append(dict(log=name, doc=i, n=len(v['records']),
                                 checkpoints=compact(v['checkpoints'], MARKER_KEY[name], i == 0), rel=v['rel'],
                                 events=dict(n=len(v['events']), sha256=digest(v['events'])), pfr=v['pfr']))
            print(name, len(docs), 'docs', sum(len(d[view]['records']) for d in docs), 'records')
    with open(os.path.join(outdir, 'relpos.expected.jsonl'), 'w') as f:
        f.write(json.dumps(dict(counts=header), separators=(',', ':')) + '\n')
        for r in rows:
            f.write(json.dumps(r, separators=(',', ':')) + '\n')
    print(json.dumps(header))


if __name__ == '__main__':
    main(*sys.argv[1:2])
