"""Marker-relative ops through the Node surface (js/batchClient.js over the N-API addon): BatchClient.applyMsg
replays the reference farm's messages, relative ops included, to the reference's states; an editing
BatchClient's annotateMarker returns the reference's op and reaches the reference's states after the acks;
posFromRelativePos gives the reference's answers (tests/golden/relpos.expected.jsonl)."""
import json
import os
import shutil
import subprocess
import sys

import pytest

from conftest import GOLDEN, REPO
from test_relpos import MARKER_KEY, fixture

sys.path.insert(0, GOLDEN)
from make_relpos import by_name, digest  # noqa: E402

NODE = shutil.which('node')
pytestmark = pytest.mark.skipif(not NODE, reason='node not installed')


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['relpos', 'relpos_c1', 'relpos_wide'])
def test_batchclient_replays_relative_ops(name):
    from fluidframework_amd import build
    build.build()
    assert build.build_napi()
    rows = fixture()[1][name]
    cmd = [NODE, os.path.join(REPO, 'js', 'replay_relpos.js'), os.path.join(GOLDEN, name + '.mtlog'),
           os.path.join(GOLDEN, 'relpos.expected.jsonl'), name, str(MARKER_KEY[name])]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    got = [json.loads(x) for x in out.stdout.strip().split('\n')]
    assert [g['doc'] for g in got] == [r['doc'] for r in rows]
    for g, r in zip(got, rows):
        assert g['err'] is None, (name, r['doc'], g['err'])
        assert [k for k, _ in g['states']] == [c['k'] for c in r['checkpoints']]
        for (k, st), c in zip(g['states'], r['checkpoints']):
            for seg in st['segs']:
                seg[5].sort()   # (the host lists an overlap set in its own short-id order)
            assert digest(st) == c['named'], (name, r['doc'], k)
            if 'state' in c:
                assert st == by_name(c['state'], MARKER_KEY[name]), (name, r['doc'], k)
        assert g['pfr'] == [q[5] for q in r['pfr']], (name, r['doc'])
        if name == 'relpos_c1':
            assert g['ops'] > 10, (r['doc'], g['ops'])   # annotateMarker ops compared with the reference's


def test_record_form_of_relative_ops():
    """_record on a stand-in engine (no device): the type bits, the blocks at the payload's tail, GROUP
    members included; `register` and non-rewrite combining ops still throw."""
    src = r"""
const { BatchEngine } = require('./js/batchClient.js');
const eng = Object.create(BatchEngine.prototype);
Object.assign(eng, { labelDecl: [], recording: false, pending: 0 });
const { BatchClient } = require('./js/batchClient.js');
const c = new BatchClient(eng, 0);
const msg = { sequenceNumber: 5, referenceSequenceNumber: 4, minimumSequenceNumber: 0 };
c._record(msg, { type: 0, pos1: 0, seg: { marker: { refType: 1 }, props: { k: 1, markerId: 'a' } } }, 1, false);
let r = c._record(msg, { type: 2, props: { k: 2 }, relativePos1: { id: 'a', before: true }, relativePos2: { id: 'a' } }, 1, false);
if (r.type !== (2 | 8 | 16) || r.pos1 !== 0 || r.pos2 !== 0 || r.npairs !== 1) throw 'annotate ' + JSON.stringify(r);
if (r.payload.toString('hex') !== '0002' + '01010100' + '00000000' + '01000100' + '00000000') throw 'payload ' + r.payload.toString('hex');
r = c._record(msg, { type: 1, relativePos1: { id: 'a', before: true, offset: 2 }, pos2: 9 }, 1, false);
if (r.type !== (1 | 8) || r.pos2 !== 9 || r.payload.toString('hex') !== '01010100' + '02000000') throw 'remove ' + r.payload.toString('hex');
r = c._record(msg, { type: 0, relativePos1: { id: 'zz', offset: -1 }, seg: 'hi' }, 1, false);
if (r.type !== (0 | 8) || r.payload.toString('hex') !== '6869' + '01000200' + 'ffffffff') throw 'insert ' + r.payload.toString('hex');
r = c._record(msg, { type: 2, pos1: 1, pos2: 2, props: { k: 2 }, relativePos1: { id: 'a' } }, 1, true);
if (r.type !== 2 || r.payload.length !== 2 || !(r.flags & 4)) throw 'an absolute end wins (getValidOpRange)';
for (const bad of [{ type: 1, relativePos1: { id: 'a' }, relativePos2: { id: 'a' }, register: 'x' },
    { type: 0, relativePos1: { id: 'a' }, register: 'x' },
    { type: 2, props: { k: 1 }, relativePos1: { id: 'a' }, relativePos2: { id: 'a' }, combiningOp: { name: 'incr', defaultValue: 1 } }]) {
    let threw = false;
    try { c._record(msg, bad, 1, false); } catch (e) { threw = true; }
    if (!threw) throw 'accepted ' + JSON.stringify(bad);
}
console.log('ok');
"""
    out = subprocess.run([NODE, '-e', src], capture_output=True, text=True, cwd=REPO, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == 'ok', out.stderr[-2000:] + out.stdout
