#!/usr/bin/env python3
"""findTile / getStackContext fixtures FROM THE REFERENCE ITSELF, asked at checkpoints in the middle of
editing, wide and observer logs (build container only; needs node and the reference's transpile under
oracle/_tsref).

tests/golden/tileforms_ref.js runs a farm of reference Clients behind a toy sequencer and logs what one
client sees (the pattern of localw_ref.js).  About a third of the inserts are markers (Tile, NestBegin,
NestEnd) with referenceTileLabels / referenceRangeLabels arrays over L0..L3 -- a record's value id is the
bitmask of its labels (js/mtlog.js tileLabels), 1..15 -- and annotates (plain, rewrite, null; remote and the
logged client's own) change those labels.  At message boundaries -- after every label annotate, on both
sides of the ack of the logged client's own label annotate, and spread over the log -- the logged client
answers findTile(p, "L"+l, preceding) and getStackContext(p, ["L"+l]) for l in 0..3 at the positions
0, 1, 2, len>>3, len>>2, len>>1, 3len>>2, len-2, len-1, len, len+1 and around the markers touched since the
previous checkpoint (at most 24 positions).  Beside each reference answer stands the PLAIN answer: the
script's own flat walk over the client's leaves with their current labels.  Where the two differ the
reference answered from a block's caches that a label annotate left stale (annotateRange refreshes no
block, mergeTree.ts:2565-2605): what MT_SF_STALE and `slab` track on the device.

  tf_scenarios       hand-written: editing documents of ten tiles over three leaf blocks -- (a) a local label
                     annotate, a checkpoint, its ack alone, a checkpoint; (b) a remote annotate of the tile
                     while the local one is pending; (c) a pending local tile insert; (d) a pending local
                     removal of a tile, then the remote removal that replaces it; (e) range labels: (a) and (c)
                     with nested begins and ends; (f) an observer document of tiles_annot's first shape asked
                     after each of its annotates
  tf_edit            an editing client, everyone catches up each round
  tf_edit_lag        the editing client lags
  tf_edit_reconnect  the reconnect farm (regenerated ops, seq -2 records)
  tf_edit_offline    more than 64 edits pending at once
  tf_wide            observer documents past the narrow limits: tile labels on key 20, range labels on key
                     27, UTF-16 text, client ids 70 and 300, other keys' value ids up to 65535
  tf_edit_wide       the same content with an editing client; its last two documents start narrow and turn
                     wide with the editing client's own label annotate pending (`promote`: {k, pending})

<log>.mtlog: the records.  tileforms.expected.jsonl: a first row {counts: {log: {...}}}, then one row per
document {log, doc, name, ids, observer, keys: [tile key, range key], n, promote, counts, checkpoints}.  A
checkpoint is {k, len, why, pend: [edits pending, label annotates pending], removed, ptile, pos, tiles:
[reference, plain], stacks: [reference, plain]} as tileforms_ref.js documents it, in full for each log's
first two documents -- the plain column kept where it differs from the reference's, as [[index, plain
answer], ...], which keeps the file a third the size; for the others `tiles` and `stacks` are replaced by
`check`, 16 hex digits of the SHA-256 of json.dumps([tiles[0], stacks[0]]) (the reference's answers).
Per-log counts: stale_differs (reference answer != plain answer; stale_differs_full: in the fully recorded
documents), ack_flips (answers that differ between the two checkpoints around a step that
holds only the ack of a local label annotate), pending_tile (answers naming a tile the logged client
inserted and that is not acked), pending_removed (checkpoints with a tile locally removed and unacked),
label_pending (checkpoints with a label annotate of the logged client pending).  tileforms.summary.json:
runs tried / kept / dropped per log and the farm's own counts.  Fixtures are data only.
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
LOGS = (('tf_scenarios', 'scenarios', 0, 6, 0), ('tf_edit', 'edit', 211, 4, 100), ('tf_edit_lag', 'edit_lag', 212, 4, 100),
        ('tf_edit_reconnect', 'edit_reconnect', 213, 4, 100), ('tf_edit_offline', 'edit_offline', 214, 4, 150),
        ('tf_wide', 'wide', 215, 4, 100), ('tf_edit_wide', 'edit_wide', 216, 4, 100))
FULL_DOCS = 2
MIN_CHECKPOINTS = 8


def dumps(x):
    return json.dumps(x, separators=(',', ':'))


def digest(tiles, stacks):
    """A checkpoint's answers, [tile positions, stacks] (the reference's, or an engine's), as 16 hex digits."""
    return hashlib.sha256(dumps([tiles, stacks]).encode()).hexdigest()[:16]


def sparse(ref, plain):
    """The plain column beside the reference's: [[index, plain answer], ...] where the two differ."""
    assert len(ref) == len(plain)
    return [[i, b] for i, (a, b) in enumerate(zip(ref, plain)) if a != b]


def differs(ck):
    """Answers of a checkpoint where the reference and the plain walk disagree."""
    return len(sparse(*ck['tiles'])) + len(sparse(*ck['stacks']))


def tuples(records):
    return [(s, r, m, c, t, p1, p2, text, None if props is None else {int(k): v for k, v in props.items()}, flags)
            for (s, r, m, c, t, p1, p2, text, props, flags) in records]


def main(outdir=HERE):
    from fluidframework_amd.oplog import build_batch
    summary, rows, head = {}, [], {}
    for log, kind, seed, n_docs, edits in LOGS:
        res = subprocess.run(['node', os.path.join(HERE, 'tileforms_ref.js'), kind, str(seed), str(n_docs), str(edits)],
                             check=True, capture_output=True, text=True)
        *docs, tail = [json.loads(x) for x in res.stdout.strip().split('\n')]
        assert tail['kept'] == n_docs, (log, tail)
        counts = {}
        for d in docs:
            for k, v in d['counts'].items():
                counts[k] = max(counts.get(k, 0), v) if k == 'pendingMax' else counts.get(k, 0) + v
        summary[log] = dict(tail, counts=counts, records=[len(d['records']) for d in docs], segs=[d['segs'] for d in docs],
                            checkpoints=[len(d['checkpoints']) for d in docs])
        build_batch([tuples(d['records']) for d in docs]).save(os.path.join(outdir, log + '.mtlog'))
        c = dict(stale_differs=0, stale_differs_full=0, ack_flips=counts['ackFlips'], pending_tile=0, pending_removed=0,
                 label_pending=0, checkpoints=0, answers=0)
        for i, d in enumerate(docs):
            cks = []
            assert len(d['checkpoints']) >= (MIN_CHECKPOINTS if kind != 'scenarios' else 4), (log, i)
            for ck in d['checkpoints']:
                c['stale_differs'] += differs(ck)
                c['stale_differs_full'] += differs(ck) if i < FULL_DOCS else 0
                c['pending_tile'] += ck['ptile']
                c['pending_removed'] += 1 if ck['removed'] else 0
                c['label_pending'] += 1 if ck['pend'][1] else 0
                c['checkpoints'] += 1
                c['answers'] += len(ck['tiles'][0]) + len(ck['stacks'][0])
                out = {k: ck[k] for k in ('k', 'len', 'why', 'pend', 'removed', 'ptile', 'pos')}
                if i < FULL_DOCS:
                    out['tiles'] = [ck['tiles'][0], sparse(*ck['tiles'])]
                    out['stacks'] = [ck['stacks'][0], sparse(*ck['stacks'])]
                else:
                    out['check'] = digest(ck['tiles'][0], ck['stacks'][0])
                cks.append(out)
            rows.append(dumps(dict(log=log, doc=i, name=d['name'], ids=d['ids'], observer=d['observer'], keys=d['keys'],
                                   n=len(d['records']), promote=d['promote'], counts=d['counts'], checkpoints=cks)))
        head[log] = c
        print(log, 'tried', tail['tried'], 'kept', tail['kept'], 'dropped', tail['dropped'],
              sum(len(d['records']) for d in docs), 'records', c)
    with open(os.path.join(outdir, 'tileforms.expected.jsonl'), 'w') as f:
        f.write('\n'.join([dumps(dict(counts=head))] + rows) + '\n')
    with open(os.path.join(outdir, 'tileforms.summary.json'), 'w') as f:
        f.write(json.dumps(summary, indent=1, sort_keys=True) + '\n')


if __name__ == '__main__':
    main(*sys.argv[1:2])
