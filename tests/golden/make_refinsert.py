#!/usr/bin/env python3
"""insertAtReferencePositionLocal fixtures FROM THE REFERENCE ITSELF (build container only; needs the
reference's transpile under oracle/_tsref and node).

tests/golden/refinsert_ref.js runs reference Clients: hand-written scenarios (the smallest documents at
which the device path can go wrong: block-first children, splits, updateRoot, pending runs past a
64-leaf window, acked tombstones, detached references, a marker with an id, every editing form) and a
farm of 4 clients, 300 ops a run, in which c1 holds up to 24 local references and makes 30 % of its
edits at one of them -- 40 runs in which every client catches up each round, 40 in which c1 lags.

  refinsert.mtlog         the scenarios as c1 sees them, one document each
  refinsert_rounds.mtlog  the farm's catching-up runs      refinsert_lag.mtlog   its lagging runs
  refinsert.expected.jsonl  first row {counts, dropped}; then one row per (log, doc):
      {log, doc, name, n, refs, ats, checkpoints[, marker]}   (refinsert_ref.js documents the fields)
An insertAtReferencePositionLocal is a local record of type 5 whose pos1 is the fixture's reference id.
Kept small (pack_at / unpack below): a state is its canonical checksum (oracle/canon.py, what
mt_checksums computes), the end's with its tree, in full up to 40 segments (scenarios) or for each farm
log's first document; an at-row is a list, its leaf flags run-length coded, its callbacks derived, its
references [id, toPosition, ordinal, offset] (those not detached) in full for the scenarios and each farm
log's first document and as a digest elsewhere.
Fixtures are data only (inputs and reference outputs).
"""
import hashlib
import json
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

F_PROPS, INSERT_AT = 2, 5
FARMS = (('refinsert_rounds', 47, 0), ('refinsert_lag', 43, 1))  # (log, seed, c1 lags)
RUNS, OPS = 40, 300
FULL_STATE_SEGS = 40
# over the 80 runs: about half of what 200 runs of each kind gave when the feature was specified
BARS = dict(applied=600, split=150, left=400, differs=10, first=60, zero=10, detached=400)
MAX_DROPPED = {'refinsert_rounds': 0, 'refinsert_lag': RUNS // 5}


def tuples(records):
    out = []
    for (s, r, m, c, t, p1, p2, text, props, flags) in records:
        props = None if props is None else {int(k): v for k, v in props.items()}
        if t == INSERT_AT and props is not None:
            flags |= F_PROPS
        out.append((s, r, m, c, t, p1, p2, text, props, flags))
    return out


def compact_state(state, full):
    from oracle.canon import checksum
    row = dict(checksum='%016x' % checksum(state), tree=state['tree'])
    if full:
        row['state'] = state
    return row


FLAGS = (('split', 's'), ('left', 'l'), ('moved', 'm'), ('zero', 'z'), ('first', 'b'), ('differs', 'd'))


def rle(flags):
    """'....pp.' as '4.2p1.'"""
    out, i = '', 0
    while i < len(flags):
        j = i
        while j < len(flags) and flags[j] == flags[i]:
            j += 1
        out += '%d%s' % (j - i, flags[i])
        i = j
    return out


def unrle(s):
    return ''.join(c * int(n) for n, c in re.findall(r'(\d+)(\D)', s))


def refs_digest(rows):
    """The references that are not detached, [[id, toPosition, ordinal, offset], ...], as 12 hex digits."""
    return hashlib.sha256(json.dumps(rows, separators=(',', ':')).encode()).hexdigest()[:12]


def events_of(x, seg_len):
    """The callbacks of an applied at-row (replay_ref.js's form): the SPLIT, if any, and the INSERT."""
    ev = []
    if x['split']:
        ev.append([-1, -2, [[x['refOrd'], -1, x['refOff'], None], [x['refOrd'] + 1, -1, x['sl'], None]]])
    return ev + [[-1, 0, [[x['ord'], x['op'], seg_len, None]]]]


def pack_at(a, seg_len, full_refs):
    """An at-row of refinsert_ref.js as the fixture keeps it: [k, id] for a detached reference, else
    [k, id, op, ord, n, levels, flags, refOrd, refOff, pre, refs[, sl[, extra]]]: flags one letter per true
    field of FLAGS, pre run-length coded, refs in full or as refs_digest, sl the right half's length of a
    split (else 0), extra {checksum, tree[, state]} where the driver kept the state.  The callbacks are
    not kept: they are events_of the row, checked here against the driver's."""
    if a['op'] is None:
        return [a['k'], a['id']]
    refs = [[i] + r for i, r in enumerate(a['refs']) if r != 0]
    x = dict(a, sl=a['ev'][0][2][1][2] if a['split'] else 0)
    assert events_of(x, seg_len) == a['ev'], (a['k'], a['ev'])
    extra = compact_state(a['state'], len(a['state']['segs']) <= FULL_STATE_SEGS) if 'state' in a else {}
    return [a['k'], a['id'], a['op'], a['ord'], a['n'], a['levels'], ''.join(c for f, c in FLAGS if a[f]), a['refOrd'],
            a['refOff'], rle(a['pre']), refs if full_refs else refs_digest(refs)] + ([x['sl'], extra] if extra else [x['sl']] if x['sl'] else [])


def unpack_at(p):
    """The named form of a packed at-row (`refs` a list or a digest; `ev` through events_of)."""
    if len(p) == 2:
        return dict(k=p[0], id=p[1], op=None)
    k, i, op, ord_, n, levels, flags, ref_ord, ref_off, pre, refs, sl, extra = p + [0, {}][len(p) - 11:]
    x = dict(k=k, id=i, op=op, ord=ord_, n=n, levels=levels, refOrd=ref_ord, refOff=ref_off, pre=unrle(pre), refs=refs, sl=sl)
    x.update({f: c in flags for f, c in FLAGS})
    x.update(extra)
    return x


def unpack(row):
    """A fixture row with its at-rows named and its checkpoints as [{k, checksum[, tree, state]}]."""
    cks = [dict(k=c[0], checksum=c[1]) if isinstance(c, list) else c for c in row['checkpoints']]
    return dict(row, ats=[unpack_at(p) for p in row['ats']], checkpoints=cks)


def seg_len(rec):
    return 1 if rec[9] & 128 else len(rec[7])


def compact(doc, log, index, scenario):
    ats = [pack_at(a, seg_len(doc['records'][a['k']]), scenario or index == 0) for a in doc['ats']]
    cks = doc['checkpoints']
    checkpoints = [[c['k'], compact_state(c['state'], False)['checksum']] for c in cks[:-1]]
    end = cks[-1]
    checkpoints.append(dict(k=end['k'], **compact_state(end['state'], len(end['state']['segs']) <= FULL_STATE_SEGS
                                                        if scenario else index == 0)))
    row = dict(log=log, doc=index, name=doc['name'], n=len(doc['records']), refs=doc['refs'], ats=ats, checkpoints=checkpoints)
    if doc.get('marker'):
        row['marker'] = doc['marker']
    return row


def run(*args):
    res = subprocess.run(['node', os.path.join(HERE, 'refinsert_ref.js')] + [str(a) for a in args], check=True,
                         capture_output=True, text=True)
    return [json.loads(x) for x in res.stdout.strip().split('\n')]


def main(outdir=HERE):
    from fluidframework_amd.oplog import build_batch
    rows, counts, dropped = [], {}, {}
    docs = run('scenarios')
    for d in docs:
        assert len(d['records']) <= 1250, (d['name'], len(d['records']))
    build_batch([tuples(d['records']) for d in docs]).save(os.path.join(outdir, 'refinsert.mtlog'))
    rows += [compact(d, 'refinsert', i, True) for i, d in enumerate(docs)]
    print('refinsert', len(docs), 'scenarios', sum(len(d['records']) for d in docs), 'records')
    for log, seed, lag in FARMS:
        *docs, tail = run('farm', seed, RUNS, OPS, lag)
        assert tail['tried'] == RUNS and tail['dropped'] <= MAX_DROPPED[log], (log, tail)
        dropped[log] = tail['dropped']
        for d in docs:
            assert len(d['checkpoints']) <= 5, (log, d['name'])
            for k, v in d['counts'].items():
                counts[k] = counts.get(k, 0) + v
        build_batch([tuples(d['records']) for d in docs]).save(os.path.join(outdir, log + '.mtlog'))
        rows += [compact(d, log, i, False) for i, d in enumerate(docs)]
        print(log, len(docs), 'runs', sum(len(d['records']) for d in docs), 'records')
    for k, bar in BARS.items():
        assert counts[k] >= bar, 'the farm holds %d of %s, the bar is %d: another seed' % (counts[k], k, bar)
    with open(os.path.join(outdir, 'refinsert.expected.jsonl'), 'w') as f:
        f.write(json.dumps(dict(counts=counts, dropped=dropped), separators=(',', ':')) + '\n')
        for r in rows:
            f.write(json.dumps(r, separators=(',', ':')) + '\n')
    print(json.dumps(dict(counts=counts, dropped=dropped)))


if __name__ == '__main__':
    main(*sys.argv[1:2])
