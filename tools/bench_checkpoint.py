"""Document checkpoints on the C3 shape: save every document of an engine that applied the C3 log, restore
them into a second engine, verify that both engines' checksums agree, and time it: the pack and unpack
kernels by HIP events (mt_last_checkpoint_stats) with their traffic, bytes read + bytes written per
second, next to the HBM peak, and end to end (wall clock around save_docs / restore_docs: sizing, pack,
D2H, digest / host check, H2D, unpack).  Beside it,
on the same documents in the same call and alternating with it after a warm-up of each, the only route
the engine had before: snapshots_raw + snapshot.load_docs (a summary: it coalesces, and drops heap,
needsScour and pending state).  Prints one JSON line per repetition and a summary line.

    python tools/bench_checkpoint.py [--docs 100000] [--ops 1024] [--reps 3] [--sample 2000]

--sample: documents of the snapshot route (its JSON parse runs in Python: the full 100 K would take
minutes); its time is reported for the sample and per document, never extrapolated silently.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--docs', type=int, default=100_000)
    ap.add_argument('--ops', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--sample', type=int, default=2000)
    ap.add_argument('--seed', type=int, default=7)
    a = ap.parse_args()
    from fluidframework_amd import checkpoint, snapshot
    from fluidframework_amd.engine import MergeEngine
    from fluidframework_amd.oplog import CONFIGS
    cfg = dict(CONFIGS['C3'])
    cfg.pop('n_docs')
    cfg['ops_per_doc'] = a.ops
    src = MergeEngine(a.docs, ops_per_launch=32)
    src.apply_staged(src.synthesize(seed=a.seed, **cfg))
    want = src.checksums()
    dst = MergeEngine(a.docs, ops_per_launch=32)
    k = min(a.sample, a.docs)
    rows = []
    for rep in range(a.reps + 1):  # rep 0: the warm-up of each route
        t0 = time.perf_counter()
        blob = src.save_docs()
        t1 = time.perf_counter()
        dst.restore_docs(blob)
        t2 = time.perf_counter()
        dst_stats = dst.checkpoint_stats()
        assert np.array_equal(dst.checksums(), want), 'restored checksums differ'
        t3 = time.perf_counter()
        raw, off = src.snapshots_raw(0, k)
        t4 = time.perf_counter()
        trees = [json.loads(bytes(raw[off[i]:off[i + 1]]).decode('latin-1')) for i in range(k)]
        snapshot.load_docs(dst, trees, doc_ids=np.arange(k, dtype=np.uint32))
        t5 = time.perf_counter()
        pack_ms, pack_b, _, _ = src.checkpoint_stats()
        _, _, unpack_ms, unpack_b = dst_stats
        row = {'rep': rep, 'pack_ms': pack_ms, 'unpack_ms': unpack_ms,
               # each kernel reads and writes the documents' bytes once
               'pack_traffic_GBs': 2 * pack_b / (pack_ms * 1e-3) / 1e9 if pack_ms else None,
               'unpack_traffic_GBs': 2 * unpack_b / (unpack_ms * 1e-3) / 1e9 if unpack_ms else None,
               'hbm_peak_GBs': HBM_PEAK_GBS, 'hbm_measured_GBs': 6290.0}
        row.update({ 'docs': a.docs, 'blob_bytes': int(len(blob)), 'bytes_per_doc': len(blob) / a.docs,
               'save_s': t1 - t0, 'restore_s': t2 - t1, 'save_GBs': len(blob) / (t1 - t0) / 1e9,
               'restore_GBs': len(blob) / (t2 - t1) / 1e9,
               'snapshot_docs': k, 'snapshot_extract_s': t4 - t3, 'snapshot_load_s': t5 - t4,
               'checkpoint_us_per_doc': (t2 - t0) / a.docs * 1e6, 'snapshot_us_per_doc': (t5 - t3) / k * 1e6})
        if rep:
            rows.append(row)
        print(json.dumps(row), flush=True)
    best = min(rows, key=lambda r: r['save_s'] + r['restore_s'])
    print(json.dumps({'summary': 'best of %d' % a.reps, **best}), flush=True)
    assert checkpoint.check(blob) == a.docs


if __name__ == '__main__':
    main()
