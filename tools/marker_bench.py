#!/usr/bin/env python3
"""Microbench of the marker-id query (mt_marker_positions_device; include/mtgpu.h "marker ids"): --docs
C3-shaped documents (C3 with 5 % of its inserts markers, a tenth of them carrying a property) replayed on
the device, then --per-doc queries per document -- a (key, value id) pair drawn like the log's own, in the
local view -- queries and results resident in HBM, as queries/s.  Every query passes over all of its
document's leaves whether or not a marker carries the id.  Beside it the route the hosts had before: the
whole-state read behind getMarkerFromId (mt_get_state, then a scan on the host) over --sample documents,
EXTRAPOLATED to all of them.  A sample of the device answers is checked against that route
(relpos.choose_marker / marker_position).  Prints one JSON line; its figures stand in DESIGN.md §5
"Marker-relative ops".  Run on the GPU box:
    python tools/marker_bench.py [--docs 100000] [--per-doc 2] [--sample 500]"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

from fluidframework_amd.engine import MARKER_QUERY_DTYPE, MARKER_RESULT_DTYPE, POS_LOCAL, MergeEngine  # noqa: E402
from fluidframework_amd.hipmem import DeviceBuffer  # noqa: E402
from fluidframework_amd.oplog import CONFIGS  # noqa: E402
from fluidframework_amd.relpos import choose_marker, marker_position  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--docs', type=int, default=100_000)
ap.add_argument('--per-doc', type=int, default=2)
ap.add_argument('--sample', type=int, default=500)
ap.add_argument('--reps', type=int, default=5)
a = ap.parse_args()
cfg = dict(CONFIGS['C3'])
cfg.pop('n_docs')
cfg['p_marker'] = 0.05
eng = MergeEngine(a.docs, ops_per_launch=32)
dev = eng.synthesize(seed=11, **cfg)
dev.free()
rng = np.random.default_rng(5)
n = a.docs * a.per_doc
q = np.zeros(n, dtype=MARKER_QUERY_DTYPE)
q['doc'] = np.repeat(np.arange(a.docs), a.per_doc)
q['ref_seq'] = POS_LOCAL
q['key'] = rng.integers(0, cfg['n_keys'], n)
q['value'] = rng.integers(1, cfg['n_values'] + 1, n)
dq = DeviceBuffer(q.nbytes).upload(q)
dr = DeviceBuffer(n * MARKER_RESULT_DTYPE.itemsize)


def timed(fn):
    fn()  # warm
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts)


t_dev = timed(lambda: eng.marker_positions_device(dq.ptr, n, dr.ptr))
got = dr.download(MARKER_RESULT_DTYPE, n)
segs = eng.seg_counts().astype(np.int64)

# the old route: the whole canonical state of the document, then a scan on the host
k = min(a.sample, a.docs)
t0 = time.perf_counter()
states = [eng.state(d) for d in range(k)]
t_read = time.perf_counter() - t0
t0 = time.perf_counter()
for d in range(k):
    for j in range(a.per_doc):
        i = d * a.per_doc + j
        o = choose_marker(states[d], int(q[i]['key']), int(q[i]['value']))
        want = (-1, 0) if o is None else (o, marker_position(states[d], o))
        assert (int(got[i]['ordinal']), int(got[i]['position'])) == want, (d, j)
t_scan = time.perf_counter() - t0
t_old_all = t_read / k * a.docs
print(json.dumps({'tool': 'marker_bench', 'docs': a.docs, 'queries': n, 'config': 'C3 (1024 ops), 5 % marker inserts',
                  'mean_segments_per_doc': round(float(segs.mean()), 1), 'found_fraction': round(float((got['ordinal'] >= 0).mean()), 3),
                  'queries_per_s': round(n / t_dev, 1), 'ms': round(t_dev * 1e3, 3),
                  'leaves_per_s': round(float(segs.sum()) * a.per_doc / t_dev, 1),
                  'state_read_sample_docs': k, 'state_read_ms_per_doc': round(t_read / k * 1e3, 4),
                  'state_read_s_all_docs_EXTRAPOLATED': round(t_old_all, 2),
                  'speedup_over_state_read_EXTRAPOLATED': round(t_old_all / t_dev, 1),
                  'host_scan_ms_per_query_python': round(t_scan / (k * a.per_doc) * 1e3, 4),
                  'note': 'one wave per query; wall time of the launch incl. synchronize; queries and results in HBM; '
                          'the old route is one mt_get_state per document (the read behind getMarkerFromId), timed on '
                          'the sample and extrapolated linearly; its host-side scan is not charged'}))
dq.free()
dr.free()
eng.close()
