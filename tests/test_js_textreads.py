"""Text reads through the Node surface (js/textHelper.js, BatchClient.createTextHelper and the SharedString
readers over the N-API addon's textRanges): every read of the fixture's plan
(tests/golden/textreads.expected.jsonl, from the reference's own MergeTreeTextHelper), the "*" placeholder
and getTextAndMarkers included; getText() without arguments is the whole-document read as before; and
Marker.toString / the tag fallback on a stand-in for the addon."""
import json
import os
import shutil
import subprocess

import pytest

from conftest import GOLDEN, REPO
from test_textreads import FULL_DOCS, TILE_KEY, digest, load_fixture

NODE = shutil.which('node')
pytestmark = pytest.mark.skipif(not NODE, reason='node not installed')


@pytest.mark.gpu
@pytest.mark.parametrize('name,n_docs', [('textreads_spec', 3), ('markers', 3), ('wide', 2), ('local_lag', 2), ('tiles_synth', 3)])
def test_batchclient_text_readers(name, n_docs):
    from fluidframework_amd import build
    build.build()
    assert build.build_napi()
    rows = [r for r in load_fixture()[1][name] if r['doc'] < n_docs]
    assert len(rows) == n_docs
    cmd = [NODE, os.path.join(REPO, 'js', 'replay_textreads.js'), os.path.join(GOLDEN, name + '.mtlog'),
           os.path.join(GOLDEN, 'textreads.expected.jsonl'), name, str(n_docs)]
    out = subprocess.run(cmd + ([str(TILE_KEY[name])] if name in TILE_KEY else []), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    got = [json.loads(x) for x in out.stdout.strip().split('\n')]
    assert [g['doc'] for g in got] == [r['doc'] for r in rows]
    for g, r in zip(got, rows):
        assert g['err'] is None, (name, r['doc'], g['err'])
        assert g['plain'] is True and len(g['steps']) == len(r['steps'])
        for mine, st in zip(g['steps'], r['steps']):
            if r['doc'] >= FULL_DOCS:
                assert digest(mine) == st['check'], (name, r['doc'], st['k'])
                continue
            for a, op in zip(mine, st['ops']):
                assert a == (op[5:6] if op[0] == 't' else op[5:7]), (name, r['doc'], st['k'], op[:5], a)


def test_text_helper_host_object():
    """Marker.toString's format, the "*" splice, the label cut and the <b> / <u> fallback of
    js/textHelper.js on a stand-in for the client and the addon -- no device needed."""
    src = r"""
const { TextHelper, markerToString } = require('./js/textHelper.js');
if (markerToString({ refType: 1 }) !== 'M Tile:  ') throw 'plain tile';
if (markerToString({ refType: 6, properties: {} }) !== 'M RangeBegin; RangeEnd:  {}') throw 'nest';
if (markerToString({ refType: 1, properties: { referenceTileLabels: ['a', 'b'], markerId: 'm1' } }) !==
    'M Tile (m1) : tile -- a; b {"referenceTileLabels":["a","b"],"markerId":"m1"}') throw 'labels';
if (markerToString({ refType: 2, properties: { referenceTileLabels: ['a'] } }) !== 'M RangeBegin:  {"referenceTileLabels":["a"]}') throw 'no tile';
if (markerToString({ refType: 5, properties: { referenceTileLabels: ['t'], referenceRangeLabels: ['r'] } }) !==
    'M Tile; RangeEnd: tile -- t range end -- r {"referenceTileLabels":["t"],"referenceRangeLabels":["r"]}') throw 'both';
// a stand-in document: "ab" M(tile L) "cd" M(nest) "ef"
const segs = [{ text: 'ab' }, { refType: 1, properties: { referenceTileLabels: ['L'] } }, { text: 'cd', properties: { 'font-weight': 'bold' } },
    { refType: 2 }, { text: 'ef' }];
const queries = [];
const native = { textRanges: (h, q) => {
    queries.push({ start: q.readInt32LE(4), end: q.readInt32LE(8), refSeq: q.readInt32LE(12), client: q.readUInt16LE(16), ph: q.readUInt16LE(18), flags: q.readUInt32LE(20) });
    const ph = q.readUInt16LE(18), text = ph ? 'ab' + String.fromCharCode(ph) + 'cd' + String.fromCharCode(ph) + 'ef' : 'abcdef';
    const rp = Buffer.alloc(8), mrp = Buffer.alloc(8), marks = Buffer.alloc(16);
    rp.writeUInt32LE(text.length, 4);
    if (q.readUInt32LE(20) & 1) { mrp.writeUInt32LE(2, 4); marks.writeInt32LE(1, 0); marks.writeUInt32LE(2, 4); marks.writeInt32LE(3, 8); marks.writeUInt32LE(4, 12); }
    return [Buffer.from(text, 'utf16le'), rp, marks, mrp];
} };
const client = { doc: 0, keyIds: new Map(), engine: { native, handle: null, flush() {} }, _checkError() {}, getCurrentSeq: () => 9, getClientId: () => 0,
    _descriptorAt: (o) => Object.assign({ ordinal: o }, segs[o]),
    walkSegments: (h, s, e) => { let p = 0; for (const [i, d] of segs.entries()) { const l = d.text ? d.text.length : 1; h(Object.assign({ ordinal: i }, d), p, 9, 0, (s || 0) - p, (e === undefined ? 8 : e) - p); p += l; } } };
const t = new TextHelper(client);
if (t.getText(9, 0) !== 'abcdef' || queries[0].refSeq !== -2147483648 || queries[0].end !== 2147483647 || queries[0].flags !== 0) throw 'local view';
if (t.getText(4, 3, ' ', 1, 5) !== 'ab cd ef' || queries[1].refSeq !== 4 || queries[1].client !== 3 || queries[1].ph !== 32 || queries[1].start !== 1) throw 'remote view';
if (t.getText(9, 0, '*') !== 'ab\nM Tile: tile -- L {"referenceTileLabels":["L"]}cd\nM RangeBegin:  ef') throw 'star ' + JSON.stringify(t.getText(9, 0, '*'));
let r = t.getTextAndMarkers(9, 0, 'L');
if (JSON.stringify(r.parallelText) !== '["ab"]' || r.parallelMarkers.length !== 1 || r.parallelMarkers[0].ordinal !== 1) throw 'cut';
if (t.getTextAndMarkers(9, 0, 'absent').parallelText.length !== 0) throw 'absent';
client.keyIds.set('font-weight', 0);  // tags: answered on the host
const before = queries.length;
r = t.getTextAndMarkers(9, 0, 'L');
if (queries.length !== before || JSON.stringify(r.parallelText) !== '["ab"]') throw 'fallback cut';
segs[3] = { refType: 1, properties: { referenceTileLabels: ['L'] } };
r = t.getTextAndMarkers(9, 0, 'L');
if (JSON.stringify(r.parallelText) !== '["ab","<b>cd"]') throw 'tags ' + JSON.stringify(r.parallelText);
let threw = false;
try { t.getTextAndMarkers(4, 3, 'L'); } catch (e) { threw = true; }
if (!threw) throw 'fallback in a remote view';
console.log('ok');
"""
    out = subprocess.run([NODE, '-e', src], cwd=REPO, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == 'ok', out.stderr
