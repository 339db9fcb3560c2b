"""bench.py's command line on one GPU at a small shape: a plain run carries the headline
figure only and runs --steps steps (the engine's launch count says so); --dump-outputs writes the
last timed step's results, which an engine and a deli in this process reproduce from the same
arguments, sampled past its caps; --full carries every side figure (C3, C5, two ranks)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu
DOCS, OPS, SEED = 600, 160, 20261015   # SEED: bench.py's default


def _bench(*args):
    out = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '1', '--docs', str(DOCS),
                          '--ops', str(OPS)] + list(args), capture_output=True, text=True, timeout=240, cwd=REPO)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [json.loads(x) for x in out.stdout.strip().split('\n') if x.startswith('{')]
    assert len(lines) == 1, out.stdout
    return lines[0]


def _load(d):
    got = {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}
    assert all(a.dtype == np.float64 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    return got


def _halves(cs):
    return np.stack([cs >> np.uint64(32), cs & np.uint64(0xFFFFFFFF)], axis=1).astype(np.float64)


def _tickets(t):
    return np.stack([t['seq'], t['msn'], t['ref_seq'], t['status']], axis=1).astype(np.float64)


def test_plain_run_dumps_what_the_engine_computes(tmp_path):
    from fluidframework_amd.engine import MergeEngine
    from fluidframework_amd.oplog import CONFIGS
    line = _bench('--steps', '3', '--warmup', '1', '--dump-outputs', str(tmp_path / 'out'))
    one = _bench('--steps', '1', '--warmup', '0')
    assert line['steps'] == 3 and line['warmup'] == 1 and line['full'] is False
    assert line['ms_per_step'] > 0 and line['value'] > 0
    # the engine counts its kernel launches over the timed steps: three steps, three times one step's
    assert one['apply_launches'] > 0 and line['apply_launches'] == 3 * one['apply_launches']
    assert line['checksum_digest'] == one['checksum_digest']
    for k in ('roofline', 'value_hbm_resident', 'cpu_baseline', 'parity', 'slow_paths'):
        assert line[k] is None
    got = _load(str(tmp_path / 'out'))
    cfg = dict(CONFIGS['C3'])
    cfg.pop('n_docs')
    cfg['ops_per_doc'] = OPS
    eng = MergeEngine(DOCS, ops_per_launch=32)
    dev = eng.synthesize(seed=SEED, **cfg)
    eng.reset()
    eng.apply_staged(dev)
    assert np.array_equal(got['doc_index'], np.arange(DOCS))
    assert np.array_equal(got['checksums'], _halves(eng.checksums()))
    assert np.array_equal(got['seg_counts'], eng.seg_counts().astype(np.float64))
    docs = got['sample_docs'].astype(np.int64)
    assert len(docs) == 256 and np.all(np.diff(docs) > 0) and docs[-1] < DOCS
    assert np.array_equal(got['sample_length'], [float(eng.length(int(d))) for d in docs])
    assert not got['sample_error'].any()
    dev.free()
    eng.close()


def test_plain_c5_run_dumps_its_tickets(tmp_path, monkeypatch):
    """The dumped tickets are those of the host-fed step run in this process, which in document
    order are those of an independent ticketing of the whole raw stream (ticket_device); past its
    caps the dump is a fixed sample of the same rows."""
    import bench
    from fluidframework_amd.deli import RAW_DTYPE, TICKET_DTYPE, DeliSequencer, batch_device_ptrs
    from fluidframework_amd.engine import MergeEngine
    from fluidframework_amd.hipmem import DeviceBuffer
    from fluidframework_amd.oplog import CONFIGS
    from fluidframework_amd.ticks import TickLog
    line = _bench('--config', 'C5', '--steps', '2', '--warmup', '1', '--dump-outputs', str(tmp_path / 'out'))
    assert line['steps'] == 2 and line['deli'] is None
    got = _load(str(tmp_path / 'out'))

    cfg = dict(CONFIGS['C5'])
    cfg.pop('n_docs')
    cfg['ops_per_doc'] = OPS
    n_join = cfg['n_clients']      # C5: the ClientJoin of its 8 clients, then its op messages
    eng = MergeEngine(DOCS, ops_per_launch=32)
    dev = eng.synthesize(seed=SEED, **cfg)
    d_ops, _, d_row = batch_device_ptrs(dev)
    deli = DeliSequencer(DOCS)
    n_msgs = dev.n_ops + DOCS * n_join
    assert n_msgs == DOCS * (OPS + n_join)
    d_msgs, d_mrow = DeviceBuffer(n_msgs * RAW_DTYPE.itemsize), DeviceBuffer((DOCS + 1) * 4)
    d_tick = DeviceBuffer(n_msgs * TICKET_DTYPE.itemsize)
    deli.raw_stream(d_ops, d_row, DOCS, n_join, d_msgs.ptr, d_mrow.ptr)
    deli.sync()
    log = TickLog.from_batch(dev.to_host(), 32, msgs=d_msgs.download(RAW_DTYPE, n_msgs),
                             msg_row_ptr=d_mrow.download(np.uint32, DOCS + 1), tickets=True)
    eng.reset()
    deli.restore_all(seq=0, clients={})
    eng.apply_ticks(log, deli=deli)
    cs = eng.checksums()
    fed = np.array(log.tickets)
    assert np.array_equal(got['sample_ticket_index'], np.arange(n_msgs))   # fewer than the cap: all of them
    assert np.array_equal(got['sample_tickets'], _tickets(fed))
    assert np.array_equal(got['checksums'], _halves(cs))

    # the same stream ticketed in one call, document-major: tick t holds document d's messages
    # [msg_row_ptrs[t][d], msg_row_ptrs[t][d + 1]) of the tick's block
    deli.restore_all(seq=0, clients={})
    deli.ticket_device(d_msgs.ptr, d_mrow.ptr, DOCS, d_tick.ptr, d_ops, dev.n_ops)
    deli.sync()
    want = d_tick.download(TICKET_DTYPE, n_msgs)
    per_doc = [[] for _ in range(DOCS)]
    for t in range(log.n_ticks):
        rp = log.msg_row_ptrs[t * (DOCS + 1):(t + 1) * (DOCS + 1)].astype(np.int64) + int(log.tick_msgs[t])
        for d in range(DOCS):
            per_doc[d].append(fed[rp[d]:rp[d + 1]])
    doc_major = np.concatenate([x for rows in per_doc for x in rows])
    assert np.all(want['status'] == 1)
    assert np.array_equal(_tickets(doc_major), _tickets(want))

    # past the caps: a fixed seeded sample, the same from call to call
    monkeypatch.setattr(bench, 'DUMP_SAMPLE_TICKETS', 1000)
    monkeypatch.setattr(bench, 'DUMP_MAX_DOCS', 100)
    for name in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / name), eng, cs, fed)
    a, b = _load(str(tmp_path / 'a')), _load(str(tmp_path / 'b'))
    assert sorted(a) == sorted(got) and all(np.array_equal(a[k], b[k]) for k in a)
    idx, rows = a['sample_ticket_index'].astype(np.int64), a['doc_index'].astype(np.int64)
    assert len(idx) == 1000 and np.all(np.diff(idx) > 0) and idx[-1] < n_msgs
    assert np.array_equal(a['sample_tickets'], _tickets(fed[idx]))
    assert len(rows) == 100 and np.all(np.diff(rows) > 0) and rows[-1] < DOCS
    assert np.array_equal(a['checksums'], _halves(cs)[rows])
    assert np.array_equal(a['seg_counts'], eng.seg_counts()[rows].astype(np.float64))
    log.free()
    dev.free()
    eng.close()


@pytest.mark.parametrize('args', [
    ('--cpu-seconds', '2'),
    ('--config', 'C5', '--no-cpu-baseline'),
    ('--config', 'C5', '--no-cpu-baseline', '--gpus', '2', '--comm', 'gloo', '--devices', '0,0'),
], ids=['C3', 'C5', 'C5-two-ranks'])
def test_full_run_carries_the_side_figures(args):
    """--full also runs bench's own checks: the host-fed steps equal the HBM-resident replay, every
    ticket of the HBM-resident steps is SENT."""
    line = _bench('--full', '--steps', '1', '--warmup', '1', *args)
    assert line['full'] is True and line['steps'] == 1
    assert line['n_gpus'] == (2 if '--gpus' in args else 1)
    assert line['roofline']['kernel'] and line['roofline']['avg_launch_ms'] > 0
    assert line['value_hbm_resident']['value'] > 0
    assert line['doc_errors_sampled'] == 0
    assert line['slow_paths'] is None   # the side lines belong to the default shape
    if 'C5' in args:
        assert line['deli']['messages_per_step'] > 0 and line['deli']['kernel_ms_per_step'] > 0
        assert line['cpu_baseline'] is None
    else:
        assert line['parity']['docs_checked'] == DOCS and line['parity']['mismatches'] == 0
        assert line['cpu_baseline']['value'] > 0
