"""Document checkpoints on the C3 shape: save every document of an engine that applied the C3 log, restore
them into a second engine, verify that both engines' checksums agree, and time it: the pack and unpack
kernels by HIP events (mt_last_checkpoint_stats) with their traffic, bytes read + bytes written per
second, next to the HBM peak, and end to end (wall clock around save_docs / restore_docs: sizing, pack,
D2H, digest / host check, H2D, unpack).  Beside it,
on the same documents in the same call and alternating with it after a warm-up of each, the only route
the engine had before: snapshots_raw + snapshot.load_docs (a summary: it coalesces, and drops heap,
needsScour and pending state).  Prints one JSON line per repetition and a summary line.

    python tools/bench_checkpoint.py [--docs 100000] [--ops 1024] [--reps 3] [--sample 2000]
    python tools/bench_checkpoint.py --editing [--docs 32768] [--reps 3]

--editing: editing clients' documents with edits pending instead (the local_big farm log tiled): the pack
and unpack kernels and the end-to-end save and restore, reported alone.

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


def editing(a):
    """--editing: the reference farm's local_big logs tiled over --docs documents (tools/bench_local.py),
    each cut in its first half where most of its editing client's edits are pending; every document saved
    and restored into a second engine.  One JSON line per repetition (rep 0: the warm-up) and a summary.
    There is no other route to compare with: a snapshot cannot carry an editing client."""
    from fluidframework_amd import checkpoint
    from fluidframework_amd.engine import MergeEngine
    from fluidframework_amd.oplog import OpBatch
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = OpBatch.load(os.path.join(here, 'tests', 'golden', 'local_big.mtlog'))
    cut = np.zeros(src.n_docs, dtype=np.int64)
    for d in range(src.n_docs):
        ops = src.ops[int(src.row_ptr[d]):int(src.row_ptr[d + 1])]
        own = int(ops['client'][ops['seq'] == -1][0])
        pend = np.cumsum((ops['seq'] == -1).astype(np.int64) - ((ops['seq'] > 0) & (ops['client'] == own)))
        cut[d] = int(np.argmax(pend[:len(ops) // 2])) + 1
    docs = a.docs if a.docs else 32768
    pick = np.arange(docs) % src.n_docs
    idx = np.concatenate([np.arange(int(src.row_ptr[p]), int(src.row_ptr[p]) + cut[p]) for p in pick])
    rp = np.concatenate([[0], np.cumsum(cut[pick])]).astype(np.uint32)
    eng = MergeEngine(docs, ops_per_launch=32)
    eng.apply(OpBatch(src.ops[idx].copy(), src.payload, rp))
    assert all(eng.error(d) == (0, 0) for d in range(0, docs, 97))
    want = eng.checksums()
    dst = MergeEngine(docs, ops_per_launch=32)
    rows = []
    for rep in range(a.reps + 1):
        t0 = time.perf_counter()
        blob = eng.save_docs()
        t1 = time.perf_counter()
        dst.restore_docs(blob)
        t2 = time.perf_counter()
        assert np.array_equal(dst.checksums(), want), 'restored checksums differ'
        pack_ms, pack_b, _, _ = eng.checkpoint_stats()
        _, _, unpack_ms, unpack_b = dst.checkpoint_stats()
        row = {'mode': 'editing', 'rep': rep, 'docs': docs, 'records_applied': int(rp[-1]), 'pack_ms': pack_ms,
               'unpack_ms': unpack_ms, 'pack_bytes': int(pack_b), 'unpack_bytes': int(unpack_b),
               'pack_traffic_GBs': 2 * pack_b / (pack_ms * 1e-3) / 1e9 if pack_ms else None,
               'unpack_traffic_GBs': 2 * unpack_b / (unpack_ms * 1e-3) / 1e9 if unpack_ms else None,
               'blob_bytes': int(len(blob)), 'bytes_per_doc': len(blob) / docs, 'save_s': t1 - t0, 'restore_s': t2 - t1}
        if rep:
            rows.append(row)
        print(json.dumps(row), flush=True)
    # (describe checks the whole blob per call: a sample through a blob of its own)
    desc = checkpoint.describe(eng.save_docs(docs=np.arange(min(docs, 64), dtype=np.uint32)))
    assert np.array_equal(dst.save_docs(docs=np.arange(min(docs, 64), dtype=np.uint32)),
                          eng.save_docs(docs=np.arange(min(docs, 64), dtype=np.uint32)))
    best = min(rows, key=lambda r: r['save_s'] + r['restore_s'])
    print(json.dumps({'summary': 'best of %d' % a.reps, **best,
                      'sample_docs': len(desc), 'sample_editing': sum('editing' in x['classes'] for x in desc),
                      'sample_pending_docs': sum(x['pending'] > 0 for x in desc),
                      'sample_pending_mean': sum(x['pending'] for x in desc) / len(desc)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--docs', type=int, default=0, help='default: 100000, with --editing 32768')
    ap.add_argument('--ops', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--sample', type=int, default=2000)
    ap.add_argument('--seed', type=int, default=7)
    ap.add_argument('--editing', action='store_true', help="editing clients' documents, edits pending")
    a = ap.parse_args()
    if a.editing:
        return editing(a)
    a.docs = a.docs or 100_000
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
