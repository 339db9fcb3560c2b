#!/usr/bin/env python3
"""Text-read fixtures FROM THE REFERENCE ITSELF (build container only; needs the reference and node).

tests/golden/textreads_ref.js replays the first documents of committed logs on a reference Client (the
transpile of oracle/tsref/build_ref.py) and, at message boundaries spread over each document, follows a
plan drawn here from a seeded PRNG of createTextHelper().getText / getTextAndMarkers calls: the whole
text, a viewport of 1-80 units, a point range, start < 0, end past the length, start > end inside one
long segment, end <= 0, each with the placeholders "", " " and "*" in turn; getTextAndMarkers with a
label the log uses and with one it does not; on observer documents also the views (refSeq, client) of
clients' latest ops' own pairs.  Editing documents (local_lag) are read in the local view only, with edits pending.
textreads_spec.mtlog is hand-written (written here too): one 200-unit segment among short ones, a
document of more than 129 short leaves with markers as leaves 63 and 64 and removed leaves at the chunk
edges, and a document that starts empty.

textreads.expected.jsonl, one row per document: {log, doc, err, steps: [{k, ops}]} as textreads_ref.js
documents them, in full for the first documents of each log; for the others each step's outputs are one
SHA-256 (`check`) and its ops keep their inputs only.  The first row holds the counts, among them
swap_nonempty: the start > end reads that returned text (above zero, or the plan does not pin
String.substring's argument swap).  Fixtures are data only (inputs and reference outputs).
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

LOGS = ('textreads_spec', 'scenarios', 'markers', 'wide', 'synth_c3', 'local_lag', 'tiles_synth')
TILE_KEY = {'tiles_synth': 0}   # the log's "referenceTileLabels" key id (js/mtlog.js)
DOCS = 4        # documents per log (the first ones)
FULL_DOCS = 2   # of which in full
STEPS = 10      # steps per document
SEED = 20240702
KINDS = ('all', 'viewport', 'point', 'neg', 'past', 'swap', 'endle0')
PLACEHOLDERS = ('', ' ', '*')
N_INPUT = {'t': 5, 'm': 5}  # fields of an op that are inputs (the rest: the reference's outputs)
COUNTS = ('reads', 'all', 'viewport', 'point', 'neg', 'past', 'swap', 'swap_nonempty', 'endle0', 'star', 'star_markers',
          'space_markers', 'tm', 'tm_cuts', 'tm_absent', 'remote', 'remote_differs', 'pending', 'units')


def spec_log():
    """OpBatch of textreads_spec."""
    import numpy as np

    from fluidframework_amd.oplog import F_MARKER, INSERT, OP_DTYPE, REMOVE, OpBatch

    docs = []
    # one 200-unit segment among short ones, split by a later insert and partly removed
    long = ''.join(chr(65 + i % 26) for i in range(200))
    docs.append([(1, INSERT, 0, 0, 'ab', 0), (2, INSERT, 2, 0, long, 0), (1, INSERT, 202, 0, 'yz', 0),
                 (2, INSERT, 0, 0, 'Q', 0), (1, REMOVE, 1, 3, '', 0), (2, INSERT, 150, 0, 'mid', 0),
                 (1, REMOVE, 100, 120, '', 0), (2, INSERT, 50, 0, '\x02', F_MARKER)])
    # 140 short leaves (alternating clients, msn 0: none is appended to its neighbour); leaves 63 and
    # 64 are markers; then removes across the chunk edges
    ops, pos = [], 0
    for i in range(140):
        if i in (63, 64):
            ops.append((1 + i % 2, INSERT, pos, 0, '\x01', F_MARKER))
            pos += 1
        else:
            t = ''.join(chr(97 + (i + j) % 26) for j in range(1 + i % 3))
            ops.append((1 + i % 2, INSERT, pos, 0, t, 0))
            pos += len(t)
    ops += [(1, REMOVE, 120, 126, '', 0), (2, REMOVE, 250, 256, '', 0), (1, INSERT, 121, 0, 'edge', 0)]
    docs.append(ops)
    # starts empty (a step before the first message), then little text
    docs.append([(1, INSERT, 0, 0, 'x', 0), (2, INSERT, 1, 0, '\x01', F_MARKER), (1, REMOVE, 0, 1, '', 0),
                 (2, INSERT, 1, 0, 'tail', 0)])
    rows, payload, row_ptr = [], bytearray(), [0]
    for ops in docs:
        for i, (client, typ, p1, p2, text, flags) in enumerate(ops):
            b = text.encode('latin-1')
            rows.append((i + 1, i, 0, client, typ, flags, p1, p2, len(payload), len(b)))
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
        if (name, d) == ('textreads_spec', 2):
            ks = [0] + ends
        plan = []
        for i, k in enumerate(ks):
            reads = []
            for j, kind in enumerate(KINDS):
                reads.append(dict(kind=kind, u=rng.getrandbits(31), v=rng.getrandbits(31),
                                  ph=PLACEHOLDERS[(i + j) % len(PLACEHOLDERS)]))
            # getTextAndMarkers: a label the tile logs use, and one no log uses
            reads.append(dict(kind=('all', 'viewport')[i % 2], u=rng.getrandbits(31), v=rng.getrandbits(31),
                              label='L%d' % (i % 3)))
            reads.append(dict(kind='all', u=0, v=0, label='absent'))
            # remote views (textreads_ref.js takes them on observer documents only)
            for kind in ('all', 'viewport', 'swap'):
                reads.append(dict(kind=kind, u=rng.getrandbits(31), v=rng.getrandbits(31), remote=1 + rng.getrandbits(16),
                                  ph=PLACEHOLDERS[(i + len(reads)) % len(PLACEHOLDERS)]))
            plan.append(dict(k=k, reads=reads))
        plans[str(d)] = plan
    return plans


def digest(x):
    return hashlib.sha256(json.dumps(x, separators=(',', ':')).encode()).hexdigest()


def split(op):
    """(inputs, outputs) of a recorded op.  The marker strings of a "*" read stay among the inputs: the
    text is composed from them, and their property order is the reference's own insertion order."""
    return op[:N_INPUT[op[0]]] + op[6:] if op[0] == 't' else op[:N_INPUT[op[0]]], op[5:6] if op[0] == 't' else op[5:]


def hashed(step):
    """A step of a document past the first ones: its ops' outputs as one SHA-256, their inputs kept."""
    return dict(k=step['k'], check=digest([split(op)[1] for op in step['ops']]), ops=[split(op)[0] for op in step['ops']])


def generate():
    """The fixture's text (and the spec log's batch), from the reference."""
    import build_ref

    from fluidframework_amd.oplog import OpBatch
    subprocess.check_call([sys.executable, os.path.join(REPO, 'oracle/tsref/build_ref.py')], stdout=subprocess.DEVNULL)
    assert os.path.isdir(build_ref.OUT)
    driver = os.path.join(HERE, 'textreads_ref.js')
    spec = spec_log()
    out, total = [], dict.fromkeys(COUNTS, 0)
    with tempfile.TemporaryDirectory() as tmp:
        for name in LOGS:
            if name == 'textreads_spec':
                path = os.path.join(tmp, 'spec.mtlog')
                spec.save(path)
            else:
                path = os.path.join(HERE, name + '.mtlog')
            plans = drawn_plans(OpBatch.load(path), name)
            plan_path = os.path.join(tmp, 'plan.json')
            with open(plan_path, 'w') as f:
                json.dump(plans, f)
            cmd = ['node', driver, path, plan_path] + ([str(TILE_KEY[name])] if name in TILE_KEY else [])
            res = subprocess.run(cmd, check=True, capture_output=True, text=True)
            for line in res.stdout.strip().split('\n'):
                r = json.loads(line)
                assert r['err'] is None, (name, r['doc'], r['err'])
                for key in COUNTS:
                    total[key] += r['counts'][key]
                steps = r['steps'] if r['doc'] < FULL_DOCS else [hashed(s) for s in r['steps']]
                out.append(json.dumps(dict(log=name, doc=r['doc'], err=r['err'], steps=steps), separators=(',', ':')))
    for key in ('swap_nonempty', 'star_markers', 'space_markers', 'tm_cuts', 'tm_absent', 'remote_differs', 'pending'):
        assert total[key] > 0, ('the plan does not exercise this', key, total)
    head = json.dumps(dict(counts=total, seed=SEED), separators=(',', ':'))
    return '\n'.join([head] + out) + '\n', spec, total


def main():
    text, spec, total = generate()
    spec.save(os.path.join(HERE, 'textreads_spec.mtlog'))
    with open(os.path.join(HERE, 'textreads.expected.jsonl'), 'w') as f:
        f.write(text)
    print(json.dumps(total))
    print(text.count('\n'), 'rows', len(text), 'B')


if __name__ == '__main__':
    main()
