"""The committed checkpoint of editing clients' documents (tests/golden/checkpoint_v1_editing.bin: the
first four local_lag documents at their checkpoint 1, the engine's own blob, format version 1) on the
host: the checker accepts it, it describes as the listing beside it says, and it survives a file.
Nothing here needs a device."""
import hashlib
import json
import os

import numpy as np

from conftest import GOLDEN

BIN = os.path.join(GOLDEN, 'checkpoint_v1_editing.bin')


def _meta():
    with open(os.path.join(GOLDEN, 'checkpoint_v1_editing.json')) as f:
        return json.load(f)


def test_committed_editing_checkpoint_is_format_1():
    from fluidframework_amd import checkpoint
    meta = _meta()
    raw = open(BIN, 'rb').read()
    assert meta['format'] == 1 and hashlib.sha256(raw).hexdigest() == meta['sha256']
    assert checkpoint.check(raw) == len(meta['documents']) == 4
    assert checkpoint.describe(raw) == meta['documents']


def test_committed_editing_checkpoint_holds_pending_edits():
    from fluidframework_amd import checkpoint
    desc = checkpoint.describe(checkpoint.read(BIN))
    assert all('editing' in d['classes'] for d in desc)
    assert any(d['pending'] > 0 for d in desc)
    assert all(d['refs'] == 0 and d['intervals'] == 0 and d['err'] == 0 for d in desc)


def test_committed_editing_checkpoint_survives_a_file(tmp_path):
    from fluidframework_amd import checkpoint
    blob = checkpoint.read(BIN)
    path = os.path.join(str(tmp_path), 'again.bin')
    checkpoint.write(path, blob)
    assert np.array_equal(checkpoint.read(path), blob)
    assert open(path, 'rb').read() == open(BIN, 'rb').read()
