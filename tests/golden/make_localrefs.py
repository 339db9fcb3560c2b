#!/usr/bin/env python3
"""Local-reference fixtures FROM THE REFERENCE ITSELF (build container only; needs the reference and node).

tests/golden/localrefs_ref.js replays the first documents of committed logs on a reference Client (the
editing client of a local_* log, else the observer) and, at message boundaries spread over each
document, checks / removes / adds LocalReferences (localReference.ts) by a plan drawn here from a
seeded PRNG: a few references per step at positions u mod length, alternating ReferenceType.Simple and
SlideOnRemove, and now and then the removal of an older one.  localrefs_spec.mtlog is hand-written
(written here too): the four cases of client.localReference.spec.ts seen by an observer, "remove to
the end twice" (a reference slid into an `after` list, then a removal with no target:
LocalReferenceCollection.clear()'s quirk) and "slide onto a tombstone, then zamboni unlinks it".

localrefs.expected.jsonl, one row per document: {log, doc, err, steps: [{k, check, remove, add}]} with
check = [[id, toPosition(), ordinal | -1, getOffset()], ...] (localrefs_ref.js) in full for the first
documents of each log; for the others each step's check is the SHA-256 of its compact JSON.  The
first row holds the coverage counts: how many references each of the reference's movers moved.
Fixtures are data only (inputs and reference outputs).
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

LOGS = ('localrefs_spec', 'scenarios', 'markers', 'synth_c3', 'wide', 'local_lag', 'local_offline', 'local_huge')
DOCS = 4        # documents per log (the first ones)
FULL_DOCS = 2   # of which in full
STEPS = 10      # steps per document
ADDS = 3        # references added per step
SEED = 20240607
SIMPLE, SLIDE = 0, 0x40
COUNTS = ('split', 'append', 'slid_before', 'slid_after', 'detached_remove', 'detached_unlink', 'kept_by_clear')


def spec_log():
    """(OpBatch, plans) of localrefs_spec: per document [(seq, ref, msn, client, type, pos1, pos2, text)]."""
    import numpy as np

    from fluidframework_amd.oplog import INSERT, OP_DTYPE, REMOVE, OpBatch

    def five(seq0, at0):  # the spec's loop: client 1 appends "0".."4", each message's msn = seq - 1
        return [(seq0 + i, seq0 + i - 1, seq0 + i - 1, 1, INSERT, at0 + i, 0, str(i)) for i in range(5)]

    docs, plans = [], []
    # "Remove segment of non-sliding / sliding local reference", "Remove segments to end ...", "Remove all ..."
    for typ, rng, tail in ((SIMPLE, (2, 3), True), (SLIDE, (2, 3), True), (SLIDE, (2, 5), False), (SLIDE, (0, 5), False)):
        ops = five(1, 0) + [(6, 5, 5, 2, REMOVE, rng[0], rng[1], '')]
        if tail:
            ops += five(7, 4)
        docs.append(ops)
        plans.append([dict(k=5, add=[dict(pos=2, type=typ)])] + [dict(k=k) for k in range(6, len(ops) + 1)])
    # remove to the end twice: the reference slides after "abc" (an `after` list), then nothing is left
    # to slide to and clear() leaves it on its removed segment; zamboni unlinks that once the msn passes
    docs.append([(1, 0, 0, 1, INSERT, 0, 0, 'abc'), (2, 1, 0, 1, INSERT, 3, 0, 'def'), (3, 2, 0, 2, REMOVE, 3, 6, ''),
                 (4, 3, 0, 2, REMOVE, 0, 3, ''), (5, 4, 4, 1, INSERT, 0, 0, 'xy'), (6, 5, 5, 1, INSERT, 2, 0, 'z'),
                 (7, 6, 6, 1, INSERT, 3, 0, 'w')])
    plans.append([dict(k=2, add=[dict(pos=4, type=SLIDE), dict(pos=1, type=SLIDE), dict(pos=5, type=SIMPLE)])] +
                 [dict(k=k) for k in range(3, 8)])
    # slide onto a tombstone: client 3 removes "cd" without having seen client 2's removal of "ef", so in
    # its view "ef" holds `start`; locally "ef" is already removed, and zamboni unlinks it with "cd"
    docs.append([(1, 0, 0, 1, INSERT, 0, 0, 'ab'), (2, 1, 0, 1, INSERT, 2, 0, 'cd'), (3, 2, 0, 1, INSERT, 4, 0, 'ef'),
                 (4, 3, 0, 2, REMOVE, 4, 6, ''), (5, 3, 0, 3, REMOVE, 2, 4, ''), (6, 5, 5, 1, INSERT, 0, 0, 'q'),
                 (7, 6, 6, 1, INSERT, 1, 0, 'r'), (8, 7, 7, 1, INSERT, 2, 0, 's')])
    plans.append([dict(k=3, add=[dict(pos=2, type=SLIDE), dict(pos=3, type=SLIDE), dict(pos=0, type=SLIDE)])] +
                 [dict(k=k) for k in range(4, 9)])
    rows, payload, row_ptr = [], bytearray(), [0]
    for ops in docs:
        for seq, ref, msn, client, typ, p1, p2, text in ops:
            b = text.encode('latin-1')
            rows.append((seq, ref, msn, client, typ, 0, p1, p2, len(payload), len(b)))
            payload += b
        row_ptr.append(len(rows))
    batch = OpBatch(np.array(rows, dtype=OP_DTYPE), np.frombuffer(bytes(payload), dtype=np.uint8), row_ptr)
    return batch, {str(d): p for d, p in enumerate(plans)}


def drawn_plans(batch, name):
    """Steps at message boundaries spread over each of the first documents, drawn from the PRNG."""
    from fluidframework_amd.oplog import F_GROUP_MORE
    plans = {}
    for d in range(min(DOCS, batch.n_docs)):
        rng = random.Random('%d/%s/%d' % (SEED, name, d))
        x = batch.ops[batch.row_ptr[d]:batch.row_ptr[d + 1]]
        ends = [i + 1 for i in range(len(x)) if not int(x['flags'][i]) & F_GROUP_MORE]
        ks = sorted({ends[max(0, (r + 1) * len(ends) // STEPS - 1)] for r in range(STEPS)} | {ends[-1]})
        plan = []
        for i, k in enumerate(ks):
            st = dict(k=k)
            if k != ks[-1]:
                st['add'] = [dict(u=rng.getrandbits(31), type=SLIDE if (i + j) & 1 else SIMPLE) for j in range(ADDS)]
                if rng.getrandbits(1):
                    st['remove'] = [dict(u=rng.getrandbits(31))]
            plan.append(st)
        plans[str(d)] = plan
    return plans


def generate():
    """The fixture's text (and the spec log's batch), from the reference."""
    from fluidframework_amd.oplog import OpBatch
    subprocess.check_call([sys.executable, os.path.join(REPO, 'oracle/tsref/build_ref.py')], stdout=subprocess.DEVNULL)
    driver = os.path.join(HERE, 'localrefs_ref.js')
    spec, spec_plans = spec_log()
    out, total = [], dict.fromkeys(COUNTS, 0)
    with tempfile.TemporaryDirectory() as tmp:
        for name in LOGS:
            if name == 'localrefs_spec':
                path, plans = os.path.join(tmp, 'spec.mtlog'), spec_plans
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
                full = name == 'localrefs_spec' or r['doc'] < FULL_DOCS
                steps = r['steps'] if full else [
                    dict(s, check=hashlib.sha256(json.dumps(s['check'], separators=(',', ':')).encode()).hexdigest())
                    for s in r['steps']]
                out.append(json.dumps(dict(log=name, doc=r['doc'], err=r['err'], steps=steps), separators=(',', ':')))
    for key in COUNTS:
        assert total[key] > 0, ('no reference was moved this way', key, total)
    head = json.dumps(dict(coverage=total, seed=SEED), separators=(',', ':'))
    return '\n'.join([head] + out) + '\n', spec, total


def main():
    text, spec, total = generate()
    spec.save(os.path.join(HERE, 'localrefs_spec.mtlog'))
    with open(os.path.join(HERE, 'localrefs.expected.jsonl'), 'w') as f:
        f.write(text)
    print(json.dumps(total))
    print(text.count('\n'), 'rows', len(text), 'B')


if __name__ == '__main__':
    main()
