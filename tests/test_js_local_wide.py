"""An editing client on a wide document through the Node surface (js/batchClient.js over the N-API addon):
BatchClients replay localw_lag and localw_reconnect (tests/golden/make_localw.py) -- the local edits through
insertTextLocal / insertMarkerLocal / removeRangeLocal / annotateRangeLocal with string keys, the stream
through applyMsg, the reconnects through regeneratePendingOp.  The ops returned, the regenerated ops, the
callbacks delivered and the final getText() are the reference's.  Before the wide editing form, _local
threw "an editing client's document stays within the narrow limits" at the first wide edit."""
import hashlib
import json
import os
import shutil
import subprocess

import pytest

import localw
from conftest import GOLDEN, REPO
from test_js_shim import _addon, _js_state_to_log

NODE = shutil.which('node')
pytestmark = pytest.mark.skipif(not NODE, reason='node not installed')


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['localw_lag', 'localw_reconnect'])
def test_batchclient_edits_wide_documents(name):
    from fluidframework_amd.oplog import decode_record
    from oracle.canon import checksum
    assert _addon()
    out = subprocess.run([NODE, os.path.join(REPO, 'js', 'replay_local.js'), os.path.join(GOLDEN, name + '.mtlog'), 'full'],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    got = {r['doc']: r for r in (json.loads(x) for x in out.stdout.strip().split('\n'))}
    batch, rows = localw.load(name)
    gold = {g['doc']: g for g in localw.events(name)}
    n_wide = 0
    for r in rows[:2] if name == 'localw_lag' else rows[:1]:
        g = got[r['doc']]
        assert g['err'] is None, (name, r['doc'], g['err'])
        # the op each local edit returned: the record the reference's own client logged for it
        a = int(batch.row_ptr[r['doc']])
        want = []
        for o in batch.ops[a:a + r['n']]:
            if o['seq'] != -1:
                continue
            t, fl, text, props = decode_record(o, batch.payload)
            props = None if props is None else {str(k): v for k, v in props.items()}
            want.append([t, int(o['pos1']), int(o['pos2']), text, props, fl & 129])
            n_wide += bool(int(o['type']) & localw.OP_WIDE)
        assert g['ops'] == want, (name, r['doc'])
        assert g.get('regen', []) == r.get('regen', []), (name, r['doc'])
        st = _js_state_to_log(g['state'])
        assert ['%016x' % checksum(st), len(st['segs'])] == r['states'][-1][1:3], (name, r['doc'])
        if 'end' in r:
            assert st == r['end'], (name, r['doc'])
        assert localw.text_digest(g['text']) == r['states'][-1][4], (name, r['doc'])
        ev, e = g['events'], gold[r['doc']]
        if 'events' in e:
            assert ev == e['events'], (name, r['doc'])
        assert len(ev) == e['n'] and hashlib.sha256(json.dumps(ev, separators=(',', ':')).encode()).hexdigest() == \
            e['sha256'], (name, r['doc'])
    assert n_wide >= 30
