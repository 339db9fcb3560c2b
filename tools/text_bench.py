#!/usr/bin/env python3
"""Microbench of the text reads (mt_text_ranges_device; include/mtgpu.h "text reads"): --docs C3 documents
replayed on the device, then two reads of the local view per document -- a viewport of --span units at
a random position, and the whole text -- queries and results resident in HBM: the count pass, the
write pass into rows from the counts' prefix sums, and both, as queries/s and output GB/s (UTF-16
units, 2 bytes each).  Beside it the only way to answer the same queries without the kernel: a loop of
mt_get_text (one whole-state copy per document) over --sample documents, EXTRAPOLATED to all of them --
the host-side slice of the viewport is not even charged.  A sample of the device answers is checked
against that loop.  Prints one JSON line; its figures stand in DESIGN.md §7 beside the other read
paths'.  Run on the GPU box:
    python tools/text_bench.py [--docs 100000] [--span 64] [--sample 2000]"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

from fluidframework_amd.engine import MergeEngine  # noqa: E402
from fluidframework_amd.hipmem import DeviceBuffer  # noqa: E402
from fluidframework_amd.oplog import CONFIGS  # noqa: E402
from fluidframework_amd.textread import TEXT_COUNT_DTYPE, TEXT_END  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--docs', type=int, default=100_000)
ap.add_argument('--span', type=int, default=64)
ap.add_argument('--sample', type=int, default=2000)
ap.add_argument('--reps', type=int, default=5)
a = ap.parse_args()
cfg = dict(CONFIGS['C3'])
cfg.pop('n_docs')
eng = MergeEngine(a.docs, ops_per_launch=32)
dev = eng.synthesize(seed=11, **cfg)
dev.free()
all_docs = np.arange(a.docs)
lens = eng.text_lengths(eng.text_queries(all_docs, 0, TEXT_END))['units'].astype(np.int64)
rng = np.random.default_rng(5)
starts = (rng.random(a.docs) * np.maximum(lens - a.span, 1)).astype(np.int32)
# per document: the viewport, then the whole text
qs = np.concatenate([eng.text_queries(all_docs, starts, starts + a.span), eng.text_queries(all_docs, 0, TEXT_END)])
order = np.argsort(np.tile(all_docs, 2), kind='stable')
qs = qs[order]
n = len(qs)
dq = DeviceBuffer(qs.nbytes).upload(qs)
dc = DeviceBuffer(n * TEXT_COUNT_DTYPE.itemsize)
drp = DeviceBuffer(4 * (n + 1))


def timed(fn):
    fn()  # warm
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts)


t_count = timed(lambda: eng.text_ranges_device(dq.ptr, n, 0, 0, 0, 0, dc.ptr))
counts = dc.download(TEXT_COUNT_DTYPE, n)['units']
row_ptr = np.zeros(n + 1, dtype=np.uint32)
np.cumsum(counts, out=row_ptr[1:])
assert int(counts.astype(np.int64).sum()) < 2**32
drp.upload(row_ptr)
total = int(row_ptr[-1])
du = DeviceBuffer(2 * max(total, 1))
t_write = timed(lambda: eng.text_ranges_device(dq.ptr, n, drp.ptr, du.ptr, 0, 0, dc.ptr))
units = du.download('<u2', total)
assert np.array_equal(dc.download(TEXT_COUNT_DTYPE, n)['units'], counts)

# the per-document loop: mt_get_text of a sample of documents, then the slice on the host
k = min(a.sample, a.docs)
t0 = time.perf_counter()
whole = [eng.text(d) for d in range(k)]
t_loop = time.perf_counter() - t0
for d in range(k):  # (documents 0..k-1 are queries 2d, 2d + 1)
    got = [units[row_ptr[2 * d + j]:row_ptr[2 * d + j + 1]].tobytes().decode('utf-16-le', 'surrogatepass') for j in (0, 1)]
    assert got[1] == whole[d] and got[0] == whole[d][int(starts[d]):int(starts[d]) + a.span], d
t_loop_all = t_loop / k * a.docs
print(json.dumps({'tool': 'text_bench', 'docs': a.docs, 'queries': n, 'config': 'C3 (1024 ops)', 'viewport_units': a.span,
                  'output_units': total, 'mean_doc_length_units': round(float(lens.mean()), 1),
                  'queries_per_s': round(n / (t_count + t_write), 1),
                  'count_pass_queries_per_s': round(n / t_count, 1), 'write_pass_queries_per_s': round(n / t_write, 1),
                  'output_GB_per_s': round(2 * total / (t_count + t_write) / 1e9, 3),
                  'write_pass_output_GB_per_s': round(2 * total / t_write / 1e9, 3),
                  'ms_count_pass': round(t_count * 1e3, 3), 'ms_write_pass': round(t_write * 1e3, 3),
                  'get_text_loop_sample_docs': k, 'get_text_loop_ms_per_doc': round(t_loop / k * 1e3, 4),
                  'get_text_loop_s_all_docs_EXTRAPOLATED': round(t_loop_all, 2),
                  'speedup_over_get_text_loop_EXTRAPOLATED': round(t_loop_all / (t_count + t_write), 1),
                  'note': 'one wave per query; wall time of each launch incl. synchronize; queries and results in HBM; '
                          'the loop is mt_get_text per document (its whole-state copy), timed on the sample and '
                          'extrapolated linearly to all documents'}))
for b in (dq, dc, drp, du):
    b.free()
eng.close()
