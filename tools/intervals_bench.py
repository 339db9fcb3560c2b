#!/usr/bin/env python3
"""Microbench of the interval overlap query (mt_intervals_overlapping_device; include/mtgpu.h): --docs C3
documents replayed on the device, --intervals intervals on each (short ranges spread over the document,
intervalType 0 / SlideOnRemove alternating), then --queries findOverlappingIntervals queries (a random
document, a viewport of up to --span characters), queries and results resident in HBM: the count pass,
the write pass into rows from the counts' prefix sums, and both.  A sample is checked against the host
entry point.  Prints one JSON line; its queries_per_s (count pass + write pass, what one complete answer
costs) stands in DESIGN.md §7 beside mt_resolve_positions' figure (tools/bench_positions.py: one wave per
query, the same leaf pass).  Run on the GPU box:
    python tools/intervals_bench.py [--docs 100000] [--intervals 16] [--queries 1000000]"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

from fluidframework_amd.engine import POS_CONTAINING, POS_LOCAL, POS_QUERY_DTYPE, MergeEngine  # noqa: E402
from fluidframework_amd.hipmem import DeviceBuffer  # noqa: E402
from fluidframework_amd.intervals import INTERVAL_QUERY_DTYPE  # noqa: E402
from fluidframework_amd.oplog import CONFIGS  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--docs', type=int, default=100_000)
ap.add_argument('--intervals', type=int, default=16)
ap.add_argument('--queries', type=int, default=1_000_000)
ap.add_argument('--span', type=int, default=64)
ap.add_argument('--reps', type=int, default=5)
a = ap.parse_args()
cfg = dict(CONFIGS['C3'])
cfg.pop('n_docs')
eng = MergeEngine(a.docs, ops_per_launch=32)
dev = eng.synthesize(seed=11, **cfg)
dev.free()
# (nothing is applied from here on: the event buffer the references need stays empty)
eng.enable_events(per_doc=16).enable_refs(2 * a.intervals).enable_intervals(a.intervals)
q = np.zeros(a.docs, dtype=POS_QUERY_DTYPE)
q['doc'], q['pos'], q['ref_seq'], q['kind'] = np.arange(a.docs), 2**31 - 1, POS_LOCAL, POS_CONTAINING
lens = eng.resolve_positions(q)['position'].astype(np.int64)  # (a position past the view answers with its length)
rng = np.random.default_rng(5)
docs = np.repeat(np.arange(a.docs), a.intervals)
starts = (np.tile(np.arange(a.intervals), a.docs) * np.repeat(lens, a.intervals)) // a.intervals
ends = np.minimum(starts + rng.integers(0, 24, len(starts)), np.repeat(lens, a.intervals))
t0 = time.perf_counter()
hs = eng.add_intervals(docs, starts, ends, np.tile([0, 2], len(docs) // 2 + 1)[:len(docs)])
t_add = time.perf_counter() - t0
assert int(hs.max()) < a.intervals, 'an interval was refused'

qs = np.zeros(a.queries, dtype=INTERVAL_QUERY_DTYPE)
qs['doc'] = rng.integers(0, a.docs, a.queries)
qs['start'] = (rng.random(a.queries) * np.maximum(lens[qs['doc']], 1)).astype(np.int32)
qs['end'] = qs['start'] + rng.integers(0, a.span + 1, a.queries)
dq = DeviceBuffer(qs.nbytes).upload(qs)
dc = DeviceBuffer(4 * a.queries)
drp = DeviceBuffer(4 * (a.queries + 1))


def timed(fn):
    fn()  # warm
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts)


t_count = timed(lambda: eng.overlapping_intervals_device(dq.ptr, a.queries, 0, dc.ptr, 0))
counts = dc.download(np.uint32, a.queries)
row_ptr = np.zeros(a.queries + 1, dtype=np.uint32)
np.cumsum(counts, out=row_ptr[1:])
drp.upload(row_ptr)
dout = DeviceBuffer(4 * max(int(row_ptr[-1]), 1))
t_write = timed(lambda: eng.overlapping_intervals_device(dq.ptr, a.queries, drp.ptr, dc.ptr, dout.ptr))
out = dout.download(np.uint32, int(row_ptr[-1]))
assert np.array_equal(dc.download(np.uint32, a.queries), counts)
k = 4096  # the host entry point on a sample must agree
h_out, h_rp = eng.overlapping_intervals(qs['doc'][:k], qs['start'][:k], qs['end'][:k])
assert np.array_equal(h_rp, row_ptr[:k + 1]) and np.array_equal(h_out, out[:int(row_ptr[k])]), \
    'device-resident and host-staged queries differ'
print(json.dumps({'tool': 'intervals_bench', 'queries': a.queries, 'docs': a.docs, 'intervals_per_doc': a.intervals,
                  'config': 'C3 (1024 ops)', 'queries_per_s': round(a.queries / (t_count + t_write), 1),
                  'count_pass_queries_per_s': round(a.queries / t_count, 1),
                  'write_pass_queries_per_s': round(a.queries / t_write, 1),
                  'ms_count_pass': round(t_count * 1e3, 3), 'ms_write_pass': round(t_write * 1e3, 3),
                  'hits_per_query': round(float(counts.mean()), 3), 'add_intervals_per_s': round(len(docs) / t_add, 1),
                  'mean_doc_length_chars': round(float(lens.mean()), 1),
                  'note': 'one wave per query; wall time of each launch (an idle fold, the kernel) incl. synchronize; '
                          'queries and results in HBM'}))
for b in (dq, dc, drp, dout):
    b.free()
eng.close()
