"""Local references through the Node surface (js/localReference.js, BatchClient.createLocalReference /
removeLocalReference over the N-API addon): toPosition() / getSegment() / getOffset() of every reference at
every step of the fixture's plan (tests/golden/localrefs.expected.jsonl, from the reference's own
LocalReference) equal the fixture, with callbacks delivered after the batch and synchronously."""
import json
import os
import shutil
import subprocess

import pytest

from conftest import GOLDEN, REPO
from test_localrefs import load_fixture, matches

NODE = shutil.which('node')
pytestmark = pytest.mark.skipif(not NODE, reason='node not installed')


@pytest.mark.gpu
@pytest.mark.parametrize('sync', [False, True])
@pytest.mark.parametrize('name,n_docs', [('localrefs_spec', 6), ('local_lag', 1)])
def test_batchclient_local_references(name, n_docs, sync):
    from fluidframework_amd import build
    build.build()
    assert build.build_napi()
    rows = [r for r in load_fixture()[1][name] if r['doc'] < n_docs]
    assert len(rows) == n_docs
    out = subprocess.run([NODE, os.path.join(REPO, 'js', 'replay_localrefs.js'), os.path.join(GOLDEN, name + '.mtlog'),
                          os.path.join(GOLDEN, 'localrefs.expected.jsonl'), name, str(n_docs)] + (['sync'] if sync else []),
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    got = [json.loads(x) for x in out.stdout.strip().split('\n')]
    assert [g['doc'] for g in got] == [r['doc'] for r in rows]
    for g, r in zip(got, rows):
        assert g['err'] is None, (name, r['doc'], g['err'])
        assert len(g['steps']) == len(r['steps'])
        for s, st in enumerate(r['steps']):
            assert matches(st['check'], g['steps'][s]), (name, r['doc'], sync, st['k'], st['check'], g['steps'][s])
