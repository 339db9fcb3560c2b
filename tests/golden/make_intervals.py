#!/usr/bin/env python3
"""Interval-collection fixtures FROM THE REFERENCE ITSELF (build container only; needs the reference and node).

The reference's packages/dds/sequence/src/intervalCollection.ts is type-stripped (oracle/tsref/tsstrip.py)
into the git-ignored oracle/_tsref/sequence/src/, next to an empty "@fluidframework/map" stub (the file
imports only types from it).  tests/golden/intervals_ref.js then replays the first documents of committed
logs on a reference Client with a SequenceInterval collection attached and, at message boundaries spread
over each document, follows a plan drawn here from a seeded PRNG: a few queries (the whole document, one
past its end, a point, a prefix, a short range), now and then the delete of a live interval by its
current toPosition() pair, and a few adds -- intervalType 0, SlideOnRemove (one in three) and some Nest,
some ends at and past the document's length.  intervals_spec.mtlog is hand-written (written here too): a
document with removes that slide and detach, one that starts empty (intervals detached from birth), one
that takes many adds per step (more than 64 live intervals) and one that is removed from the front piece by piece.

intervals.expected.jsonl, one row per document: {log, doc, err, steps: [{k, check, ops}]} as
intervals_ref.js documents them, in full for the first documents of each log; for the others each
step's answers (every live interval's toPosition() pair and its queries' per-interval ids) are one
SHA-256 and its ops keep their inputs only.  The first row holds the counts: queries, queries where the reference's (stale) tree gave
the per-interval answer, skipped adds and deletes, how the intervals' ends moved, and the interval x
query pairs with an end on an unlinked segment.  Fixtures are data only (inputs and reference outputs).
"""
import hashlib
import json
import os
import random
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'oracle', 'tsref'))

LOGS = ('intervals_spec', 'scenarios', 'markers', 'wide', 'synth_c3', 'local_lag', 'local_offline')
DOCS = 4        # documents per log (the first ones)
FULL_DOCS = 2   # of which in full
STEPS = 10      # steps per document
ADDS = 2        # intervals added per step
QUERIES = 3     # queries per step
MANY = 24       # adds per step of the spec log's document 2
SEED = 20240611
SIMPLE, NEST, SLIDE = 0, 1, 2
KINDS = ('all', 'past', 'point', 'head', 'range')
COUNTS = ('queries', 'tree_exact', 'skipped_add_duplicate', 'skipped_add_no_at', 'skipped_delete', 'slid',
          'detached_remove', 'born_detached', 'unlinked_pairs', 'pairs', 'adds', 'deletes')
REF = os.environ.get('FLUID_REFERENCE', '/root/reference')


def build_transpile():
    """oracle/_tsref (oracle/tsref/build_ref.py) plus the sequence package's intervalCollection.ts."""
    import build_ref
    subprocess.check_call([sys.executable, os.path.join(REPO, 'oracle/tsref/build_ref.py')], stdout=subprocess.DEVNULL)
    build_ref.strip_to(os.path.join(REF, 'packages/dds/sequence/src/intervalCollection.ts'),
                       os.path.join(build_ref.OUT, 'sequence/src/intervalCollection.js'))
    stub = os.path.join(build_ref.OUT, 'node_modules/@fluidframework/map/index.js')
    os.makedirs(os.path.dirname(stub), exist_ok=True)
    with open(stub, 'w') as f:
        f.write('"use strict";\n')


def spec_log():
    """OpBatch of intervals_spec: per document [(seq, ref, msn, client, type, pos1, pos2, text)]."""
    import numpy as np

    from fluidframework_amd.oplog import INSERT, OP_DTYPE, REMOVE, OpBatch

    def seqd(ops, msn_from):  # (client, type, pos1, pos2, text) in order; msn trails by one from msn_from on
        return [(i + 1, i, i if i + 1 >= msn_from else 0, c, t, p1, p2, s) for i, (c, t, p1, p2, s) in enumerate(ops)]

    docs = []
    # removes that slide and detach, then zamboni once the msn moves
    docs.append(seqd([(1, INSERT, 0, 0, 'abcdefghij'), (1, INSERT, 5, 0, 'KLMNOP'), (2, REMOVE, 3, 8, ''),
                      (1, INSERT, 0, 0, 'xyz'), (2, REMOVE, 0, 2, ''), (1, INSERT, 12, 0, 'end'), (2, REMOVE, 4, 15, ''),
                      (1, INSERT, 4, 0, 'tail'), (1, INSERT, 0, 0, 'q'), (2, INSERT, 9, 0, 'r')], 8))
    # starts empty: the first step's intervals are detached from birth
    docs.append(seqd([(1, INSERT, 0, 0, 'one '), (2, INSERT, 4, 0, 'two '), (1, INSERT, 8, 0, 'three'), (2, REMOVE, 2, 6, ''),
                      (1, INSERT, 0, 0, 'zero '), (2, REMOVE, 0, 14, ''), (1, INSERT, 0, 0, 'again'), (1, INSERT, 5, 0, '!')], 6))
    # many intervals: long text, split over and over, partly removed
    text = ''.join(chr(97 + i % 26) for i in range(60))
    many = [(1, INSERT, 0, 0, text), (2, INSERT, 30, 0, text), (1, INSERT, 90, 0, text), (2, INSERT, 10, 0, text)]
    many += [(1 + i % 2, REMOVE, 20 + 17 * i, 29 + 17 * i, '') for i in range(4)]
    many += [(1, INSERT, 50, 0, 'MID'), (2, REMOVE, 100, 160, ''), (1, INSERT, 0, 0, 'top'), (2, INSERT, 40, 0, 'z')]
    docs.append(seqd(many, 9))
    # removed from the front, piece by piece, then refilled
    docs.append(seqd([(1, INSERT, 0, 0, 'abc'), (1, INSERT, 3, 0, 'def'), (1, INSERT, 6, 0, 'ghi'), (2, REMOVE, 0, 2, ''),
                      (2, REMOVE, 0, 3, ''), (2, REMOVE, 1, 3, ''), (1, INSERT, 0, 0, 'xy'), (1, INSERT, 2, 0, 'z'),
                      (1, INSERT, 3, 0, 'w')], 7))
    rows, payload, row_ptr = [], bytearray(), [0]
    for ops in docs:
        for seq, ref, msn, client, typ, p1, p2, text in ops:
            b = text.encode('latin-1')
            rows.append((seq, ref, msn, client, typ, 0, p1, p2, len(payload), len(b)))
            payload += b
        row_ptr.append(len(rows))
    return OpBatch(np.array(rows, dtype=OP_DTYPE), np.frombuffer(bytes(payload), dtype=np.uint8), row_ptr)


def drawn_plans(batch, name):
    """Steps at message boundaries spread over each of the first documents, drawn from the PRNG."""
    from fluidframework_amd.oplog import F_GROUP_MORE
    plans = {}
    for d in range(min(DOCS, batch.n_docs)):
        rng = random.Random('%d/%s/%d' % (SEED, name, d))
        x = batch.ops[batch.row_ptr[d]:batch.row_ptr[d + 1]]
        ends = [i + 1 for i in range(len(x)) if not int(x['flags'][i]) & F_GROUP_MORE]
        ks = sorted({ends[max(0, (r + 1) * len(ends) // STEPS - 1)] for r in range(STEPS)} | {ends[-1]})
        if name == 'intervals_spec':
            ks = ([0] if d == 1 else []) + ends
        n_adds = MANY if (name, d) == ('intervals_spec', 2) else ADDS
        plan = []
        for i, k in enumerate(ks):
            st = dict(k=k, q=[dict(kind=KINDS[(i + j) % len(KINDS)], u=rng.getrandbits(31), v=rng.getrandbits(31))
                              for j in range(QUERIES)])
            if k != ks[-1]:
                if rng.getrandbits(1):
                    st['del'] = [dict(u=rng.getrandbits(31))]
                st['add'] = [dict(u=rng.getrandbits(31), v=rng.getrandbits(31), mode=(0, 0, 0, 0, 1, 2)[rng.randrange(6)],
                                  type=NEST if (i + j) % 5 == 4 else SLIDE if (i + j) % 3 == 1 else SIMPLE)
                             for j in range(n_adds)]
            plan.append(st)
        plans[str(d)] = plan
    return plans


def digest(x):
    return hashlib.sha256(json.dumps(x, separators=(',', ':')).encode()).hexdigest()


def hashed(step):
    """A step of a document past the first ones: its answers -- [id, start toPosition(), end toPosition()]
    of every live interval, then each query's per-interval ids without the intervals that have an end on an
    unlinked segment -- as one SHA-256; its ops keep their inputs (a query also that list of intervals)."""
    answers = [[[c[0], c[3], c[6]] for c in step['check']]]
    ops = []
    for op in step['ops']:
        if op[0] == 'q':
            un = op[7] if len(op) > 7 else []
            answers.append([i for i in op[3] if i not in un])
            ops.append(op[:3] + ([un] if un else []))
        else:
            ops.append(op)
    return dict(k=step['k'], check=digest(answers), ops=ops)


def generate():
    """The fixture's text (and the spec log's batch), from the reference."""
    from fluidframework_amd.oplog import OpBatch
    build_transpile()
    driver = os.path.join(HERE, 'intervals_ref.js')
    spec = spec_log()
    out, total, max_live = [], dict.fromkeys(COUNTS, 0), 0
    with tempfile.TemporaryDirectory() as tmp:
        for name in LOGS:
            if name == 'intervals_spec':
                path = os.path.join(tmp, 'spec.mtlog')
                spec.save(path)
            else:
                path = os.path.join(HERE, name + '.mtlog')
            plans = drawn_plans(OpBatch.load(path), name)
            plan_path = os.path.join(tmp, 'plan.json')
            with open(plan_path, 'w') as f:
                json.dump(plans, f)
            res = subprocess.run(['node', driver, path, plan_path], check=True, capture_output=True, text=True)
            for line in res.stdout.strip().split('\n'):
                r = json.loads(line)
                assert r['err'] is None, (name, r['doc'], r['err'])
                for key in COUNTS:
                    total[key] += r['counts'][key]
                max_live = max(max_live, r['counts']['max_live'])
                for s in r['steps']:
                    for op in s['ops']:
                        if op[0] == 'q':
                            assert set(op[4]) <= set(op[3]), ('the tree answered an interval that does not overlap', name, op)
                steps = r['steps'] if r['doc'] < FULL_DOCS else [hashed(s) for s in r['steps']]
                out.append(json.dumps(dict(log=name, doc=r['doc'], err=r['err'], steps=steps), separators=(',', ':')))
    for key in ('slid', 'detached_remove', 'born_detached'):
        assert total[key] > 0, ('no interval end was moved this way', key, total)
    assert max_live > 64, max_live
    assert total['unlinked_pairs'] * 100 <= total['pairs'], total
    head = json.dumps(dict(counts=dict(total, max_live=max_live), seed=SEED), separators=(',', ':'))
    return '\n'.join([head] + out) + '\n', spec, dict(total, max_live=max_live)


def main():
    text, spec, total = generate()
    spec.save(os.path.join(HERE, 'intervals_spec.mtlog'))
    with open(os.path.join(HERE, 'intervals.expected.jsonl'), 'w') as f:
        f.write(text)
    print(json.dumps(total))
    print(text.count('\n'), 'rows', len(text), 'B')


if __name__ == '__main__':
    main()
