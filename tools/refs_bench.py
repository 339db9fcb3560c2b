#!/usr/bin/env python3
"""Local references on C3 with events recorded: what the tracker, the resolve and the apply cost.

C3 on --docs documents, its log in two halves (host batches): the first half applied, then
--refs references per document (alternating Simple / SlideOnRemove, spread over the document) on
--share of the documents (0, 0.01, 1), then the second half applied (timed: the apply itself, to
the device synchronise), then the tracker alone (an empty mt_refs_remove folds every document's rows;
timed to the synchronise) and the resolve (the whole mt_refs_positions call for every reference, the
rows already folded: its allocation, the copies in and out, an idle fold and the mark / resolve /
gather kernels -- not the resolve kernel alone).  --reps repetitions from a reset, the first one
warm-up; per figure the median and the min..max spread.  One JSON line per share.
    python tools/refs_bench.py [--docs 20000] [--refs 16] [--reps 4] [--shares 0,0.01,1]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
from fluidframework_amd.engine import POS_CONTAINING, POS_LOCAL, POS_QUERY_DTYPE, MergeEngine  # noqa: E402
from fluidframework_amd.hipmem import device_synchronize  # noqa: E402
from fluidframework_amd.oplog import CONFIGS, OpBatch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--docs', type=int, default=20_000)
ap.add_argument('--refs', type=int, default=16)
ap.add_argument('--reps', type=int, default=4)
ap.add_argument('--shares', default='0,0.01,1')
a = ap.parse_args()
cfg = dict(CONFIGS['C3'])
cfg.pop('n_docs')
eng = MergeEngine(a.docs, ops_per_launch=32)
eng.enable_events(per_doc=8192)
dev = eng.synthesize(seed=1, **cfg)
want = eng.checksums()
full = dev.to_host()
dev.free()
n = cfg['ops_per_doc']
halves = []
for lo, hi in ((0, n // 2), (n // 2, n)):
    idx = np.concatenate([np.arange(int(full.row_ptr[d]) + lo, int(full.row_ptr[d]) + hi) for d in range(a.docs)])
    halves.append(OpBatch(full.ops[idx].copy(), full.payload, np.arange(0, a.docs * (hi - lo) + 1, hi - lo, dtype=np.uint32)))
staged = [eng.stage(h) for h in halves]


def spread(xs):
    return dict(median=round(statistics.median(xs), 3), min=round(min(xs), 3), max=round(max(xs), 3))


for share in [float(x) for x in a.shares.split(',')]:
    eng.enable_events(per_doc=8192)  # (also frees the reference tables)
    eng.enable_refs(a.refs)
    with_refs = np.arange(a.docs)[:int(round(a.docs * share))] if share < 1 else np.arange(a.docs)
    if 0 < share < 1:
        with_refs = np.arange(0, a.docs, int(round(1 / share)))
    t_apply, t_track, t_resolve, rows_folded = [], [], [], 0
    for r in range(a.reps + 1):
        eng.reset()
        eng.drain_event_rows()
        eng.apply_staged(staged[0])
        eng.drain_event_rows()
        docs = np.repeat(with_refs, a.refs).astype(np.uint32)
        hs = np.zeros(0, np.uint32)
        if len(docs):
            # each document's local length: a position past the view answers with it (include/mtgpu.h)
            q = np.zeros(len(with_refs), dtype=POS_QUERY_DTYPE)
            q['doc'], q['pos'], q['ref_seq'], q['kind'] = with_refs, 2**31 - 1, POS_LOCAL, POS_CONTAINING
            lens = eng.resolve_positions(q)['position'].astype(np.int64)
            keep = np.repeat(lens > 0, a.refs)
            pos = (np.tile(np.arange(a.refs), len(with_refs)) * np.repeat(lens, a.refs)) // a.refs
            docs, pos = docs[keep], pos[keep]
            hs = eng.add_refs(docs, pos, np.tile([0, 0x40], len(docs) // 2 + 1)[:len(docs)])
            assert int(hs.max()) < a.refs, 'a reference was refused'
        device_synchronize()
        t0 = time.perf_counter()
        eng.apply_staged(staged[1])
        device_synchronize()
        t1 = time.perf_counter()
        eng.remove_refs(np.zeros(0, np.uint32), np.zeros(0, np.uint32))  # the fold alone
        device_synchronize()
        t2 = time.perf_counter()
        if len(docs):
            eng.ref_positions(docs, hs)
        t3 = time.perf_counter()
        _, rp = eng.drain_event_rows()
        if r:
            t_apply.append((t1 - t0) * 1e3)
            t_track.append((t2 - t1) * 1e3)
            t_resolve.append((t3 - t2) * 1e3)
            rows_folded = int(sum(int(rp[d + 1]) - int(rp[d]) for d in with_refs)) if len(with_refs) < a.docs else int(rp[-1])
    ok = bool(np.array_equal(eng.checksums(), want))
    ops = a.docs * (n - n // 2)
    out = {'tool': 'refs_bench', 'docs': a.docs, 'share': share, 'refs': int(len(docs)),
           'apply_ms': spread(t_apply), 'apply_ops_per_s': round(ops / (statistics.median(t_apply) * 1e-3), 1),
           'final_state_equals_generation': ok}
    out['track_ms'] = spread(t_track)
    out['event_rows_of_documents_with_references'] = rows_folded
    if len(docs):
        out['track_rows_per_s'] = round(rows_folded / (statistics.median(t_track) * 1e-3), 1)
        out['positions_call_ms'] = spread(t_resolve)
        out['positions_call_refs_per_s'] = round(len(docs) / (statistics.median(t_resolve) * 1e-3), 1)
    print(json.dumps(out), flush=True)
eng.close()
