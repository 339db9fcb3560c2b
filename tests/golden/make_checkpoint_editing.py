#!/usr/bin/env python
"""Regenerate checkpoint_v1_editing.bin / .json (needs the GPU): the first four local_lag documents at
their checkpoint 1, saved by the engine itself -- editing clients' documents with edits pending, format
version 1.  The listing is checkpoint.describe's, as checkpoint_v1.json is.

    python tests/golden/make_checkpoint_editing.py [--out tests/golden]
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

DOCS, CHECKPOINT = 4, 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=HERE)
    a = ap.parse_args()
    from fluidframework_amd import checkpoint
    from fluidframework_amd.engine import MergeEngine
    from fluidframework_amd.oplog import OpBatch
    batch = OpBatch.load(os.path.join(HERE, 'local_lag.mtlog'))
    with open(os.path.join(HERE, 'local.expected.jsonl')) as f:
        rows = [r for r in map(json.loads, f) if r['log'] == 'local_lag'][:DOCS]
    idx, rp = [], [0]
    for r in rows:
        base, k = int(batch.row_ptr[r['doc']]), r['states'][CHECKPOINT][0]
        idx.append(np.arange(base, base + k))
        rp.append(rp[-1] + k)
    eng = MergeEngine(DOCS, ops_per_launch=32)
    eng.apply(OpBatch(batch.ops[np.concatenate(idx)].copy(), batch.payload, np.array(rp, dtype=np.uint32)))
    for i, r in enumerate(rows):
        assert eng.error(i) == (0, 0) and eng.state(i) == r['states'][CHECKPOINT][1], r['doc']
    blob = eng.save_docs()
    eng.close()
    os.makedirs(a.out, exist_ok=True)
    checkpoint.write(os.path.join(a.out, 'checkpoint_v1_editing.bin'), blob)
    meta = {'format': 1, 'log': 'local_lag', 'cut': "checkpoint 1 of the log's first four documents",
            'sha256': hashlib.sha256(blob.tobytes()).hexdigest(), 'documents': checkpoint.describe(blob)}
    with open(os.path.join(a.out, 'checkpoint_v1_editing.json'), 'w') as f:
        json.dump(meta, f, indent=1)
        f.write('\n')
    print(len(blob), 'bytes;', sum(d['pending'] > 0 for d in meta['documents']), 'documents with edits pending')


if __name__ == '__main__':
    main()
