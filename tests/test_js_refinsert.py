"""insertAtReferencePositionLocal through the Node surface (js/batchClient.js over the N-API addon): editing
BatchClients replay the reference's scenarios and farm (tests/golden/refinsert*.mtlog), every type-5 record
through BatchClient.insertAtReferencePositionLocal at the fixture's reference.  The returned ops are the
reference's (undefined for a detached reference), the delta callback of each is the reference's INSERT with
opArgs that carry the op and no sequencedMessage, and the documents end in the reference's states."""
import json
import os
import shutil
import subprocess
import sys

import pytest

from conftest import GOLDEN, REPO
from test_refinsert import LOGS, bars, fixture, load_log, seg_len

sys.path.insert(0, GOLDEN)
from make_relpos import by_name  # noqa: E402

NODE = shutil.which('node')
pytestmark = pytest.mark.skipif(not NODE, reason='node not installed')
MARKER_KEY = 3


@pytest.mark.gpu
@pytest.mark.parametrize('name', LOGS)
def test_batchclient_inserts_at_references(name):
    from fluidframework_amd import build
    build.build()
    assert build.build_napi()
    rows = fixture()[1][name]
    cmd = [NODE, os.path.join(REPO, 'js', 'replay_refinsert.js'), os.path.join(GOLDEN, name + '.mtlog'),
           os.path.join(GOLDEN, 'refinsert.expected.jsonl'), name, str(MARKER_KEY)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    got = [json.loads(x) for x in out.stdout.strip().split('\n')]
    assert [g['doc'] for g in got] == [r['doc'] for r in rows]
    n_ops = n_states = 0
    for g, r in zip(got, rows):
        assert g['err'] is None, (name, r['doc'], g['err'])
        assert [a['op'] for a in g['ats']] == [x['op'] for x in r['ats']], (name, r['doc'])
        for a, x in zip(g['ats'], r['ats']):
            if x['op'] is None:
                assert a['cbs'] == [], (name, r['doc'], x['k'])
                continue
            want = [[e[1], [s[:3] for s in e[2]], True]
                    for e in bars().events_of(x, seg_len(load_log(name), r['doc'], x['k'])) if e[1] >= 0]
            assert a['cbs'] == want, (name, r['doc'], x['k'], a['cbs'], want)
            n_ops += 1
        end = r['checkpoints'][-1]
        assert g['state']['tree'] == end['tree'], (name, r['doc'])
        if 'state' in end:
            st = g['state']
            for seg in st['segs']:
                seg[5].sort()   # (the host lists an overlap set in its own short-id order)
            assert st == by_name(end['state'], MARKER_KEY), (name, r['doc'])
            n_states += 1
    assert n_ops >= (25 if name == 'refinsert' else 400) and n_states >= 1


def test_detached_handle_and_empty_segment_on_a_stand_in_engine():
    """Without a device: a reference that was never added (or was removed) and an empty text give undefined
    and queue nothing; a wide segment is refused as insertSegmentLocal refuses it."""
    src = r"""
const { BatchEngine, BatchClient, LocalReference } = require('./js/batchClient.js');
const eng = Object.create(BatchEngine.prototype);
Object.assign(eng, { labelDecl: [], recording: false, pending: 0, gen: 0 });
eng._enableRefs = () => { throw new Error('reached the device'); };
const c = new BatchClient(eng, 0);
let threw = false;
try { c.insertAtReferencePositionLocal(new LocalReference(c, undefined, 0, 0), 'x'); } catch (e) { threw = true; }
if (!threw) throw 'startOrUpdateCollaboration is required first';
c.startOrUpdateCollaboration('c1');
const never = new LocalReference(c, undefined, 0, 0);
if (c.insertAtReferencePositionLocal(never, 'abc') !== undefined) throw 'a reference without a handle';
never.handle = 3;
if (c.insertAtReferencePositionLocal(never, '') !== undefined) throw 'an empty segment';
threw = false;
try { c.insertAtReferencePositionLocal(never, '中'); } catch (e) { threw = /narrow/.test(e.message); }
if (!threw) throw 'a wide segment';
if (c.queue.length || eng.pending) throw 'queued something';
console.log('ok');
"""
    out = subprocess.run([NODE, '-e', src], capture_output=True, text=True, cwd=REPO, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == 'ok', out.stderr[-2000:] + out.stdout
