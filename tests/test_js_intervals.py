"""Interval collections through the Node surface (js/intervalCollection.js, BatchClient.getIntervalCollection
over the N-API addon): add, delete, findOverlappingIntervals, serializeInternal and the addInterval /
deleteInterval events at every step of the fixture's plan (tests/golden/intervals.expected.jsonl, from the
reference's own intervalCollection.ts); and the host object's labels, properties and events on a stand-in
for the addon."""
import json
import os
import shutil
import subprocess

import pytest

from conftest import GOLDEN, REPO
from test_intervals import digest, load_fixture

NODE = shutil.which('node')
pytestmark = pytest.mark.skipif(not NODE, reason='node not installed')


@pytest.mark.gpu
@pytest.mark.parametrize('name,n_docs', [('intervals_spec', 4), ('local_lag', 2)])
def test_batchclient_interval_collection(name, n_docs):
    from fluidframework_amd import build
    build.build()
    assert build.build_napi()
    rows = [r for r in load_fixture()[1][name] if r['doc'] < n_docs]
    assert len(rows) == n_docs
    out = subprocess.run([NODE, os.path.join(REPO, 'js', 'replay_intervals.js'), os.path.join(GOLDEN, name + '.mtlog'),
                          os.path.join(GOLDEN, 'intervals.expected.jsonl'), name, str(n_docs)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    got = [json.loads(x) for x in out.stdout.strip().split('\n')]
    assert [g['doc'] for g in got] == [r['doc'] for r in rows]
    for g, r in zip(got, rows):
        assert g['err'] is None, (name, r['doc'], g['err'])
        assert g['labels'] is True and len(g['steps']) == len(r['steps'])
        ops = [op for st in r['steps'] for op in st['ops']]
        assert g['events'] == dict(add=sum(op[0] == 'a' for op in ops), delete=sum(op[0] == 'd' for op in ops))
        for mine, st in zip(g['steps'], r['steps']):
            qs = [op for op in st['ops'] if op[0] == 'q']
            if isinstance(st['check'], str):
                outs = [set(op[3]) if len(op) > 3 else set() for op in qs]
                answers = [mine['check']] + [[i for i in a if i not in o] for a, o in zip(mine['q'], outs)]
                assert digest(answers) == st['check'], (name, r['doc'], st['k'])
                continue
            assert mine['check'] == [[x[0], x[3], x[6]] for x in st['check']], (name, r['doc'], st['k'])
            for a, op in zip(mine['q'], qs):
                o = set(op[7]) if len(op) > 7 else set()
                assert [i for i in a if i not in o] == [i for i in op[3] if i not in o], (name, r['doc'], st['k'], op)


def test_interval_collection_host_object():
    """Labels, properties, events and the value-type emitter of js/intervalCollection.js on a stand-in
    for the client and the addon -- no device needed."""
    src = r"""
const { IntervalCollection, IntervalType, reservedRangeLabelsKey, refTypes } = require('./js/intervalCollection.js');
if (reservedRangeLabelsKey !== 'referenceRangeLabels') throw 'key';
if (refTypes(0).join() !== '16,32' || refTypes(1).join() !== '2,4' || refTypes(2).join() !== '80,96' || refTypes(3).join() !== '80,96') throw 'refTypes';
const table = [];  // the stand-in's interval table: {start, end, coll}
const u32 = (v) => { const b = Buffer.alloc(4); b.writeUInt32LE(v, 0); return b; };
const native = {
    intervalsAdd: (h, a) => { table.push({ start: a.readInt32LE(4), end: a.readInt32LE(8), type: a.readUInt16LE(12), coll: a.readUInt16LE(14) }); return u32(table.length - 1); },
    intervalsRemove: (h, q) => {
        const i = table.findIndex((x) => x && x.start === q.readInt32LE(4) && x.end === q.readInt32LE(8) && x.coll === q.readUInt32LE(12));
        if (i >= 0) table[i] = null;
        return u32(i >= 0 ? i : 0xffffffff);
    },
    intervalsOverlapping: (h, q) => {
        const hit = table.map((x, i) => [x, i]).filter(([x]) => x && x.coll === q.readUInt32LE(12) && x.start < q.readInt32LE(8) && x.end >= q.readInt32LE(4)).map(([, i]) => i);
        const hs = Buffer.alloc(4 * hit.length + 4), rp = Buffer.alloc(8);
        hit.forEach((x, i) => hs.writeUInt32LE(x, 4 * i));
        rp.writeUInt32LE(hit.length, 4);
        return [hs, rp];
    },
};
const client = { doc: 0, engine: { native, handle: null, _enableIntervals() {}, flush() {} }, _checkError() {}, getCurrentSeq: () => 41,
    _intervalPositions: () => [table.map((x) => (x ? { start: x.start, end: x.end } : {})), table.map((x, i) => ({ startRef: 2 * i, endRef: 2 * i + 1 }))],
    _refPositions: (hs) => hs.map((h) => ({ position: h % 2 ? table[h >> 1].end : table[h >> 1].start, ordinal: 0, offset: 0 })) };
const sent = [], seen = [];
const coll = new IntervalCollection(client, 'comments', 5, { emit: (...a) => sent.push(a) });
coll.on('addInterval', (iv, local, op) => seen.push(['add', iv, local, op]));
coll.on('deleteInterval', (iv, local, op) => seen.push(['delete', iv, local, op]));
coll.add(2, 6, IntervalType.SlideOnRemove, { author: 'a', gone: 1 });
const iv = seen[0][1];
if (seen[0][2] !== true || seen[0][3] !== undefined || iv.handle !== 0 || table[0].coll !== 5 || table[0].type !== 2) throw 'add';
if (JSON.stringify(iv.properties) !== '{"referenceRangeLabels":["comments"],"author":"a","gone":1}') throw 'properties ' + JSON.stringify(iv.properties);
iv.addProperties({ gone: null });
if ('gone' in iv.getProperties()) throw 'addProperties';
if (iv.start.refType !== 0x50 || iv.end.refType !== 0x60 || iv.start.pairedRef !== iv.end || iv.start.handle !== 0 || iv.end.handle !== 1) throw 'refs';
if (iv.start.getProperties().referenceRangeLabels[0] !== 'comments') throw 'ref label';
if (sent.length !== 1 || sent[0][0] !== 'add' || sent[0][1] !== undefined || sent[0][2].start !== 2 || sent[0][2].sequenceNumber !== 41) throw 'emitter';
coll.addInternal({ start: 8, end: 9, intervalType: 0 }, false, { sequenceNumber: 50 });
if (sent.length !== 1 || seen[1][2] !== false || seen[1][3].sequenceNumber !== 50) throw 'remote add';
const des = [];
coll.attachDeserializer((x) => des.push(x));
if (des.length !== 2) throw 'deserializer';
if (coll.findOverlappingIntervals(0, 7).length !== 1 || coll.findOverlappingIntervals(0, 7)[0] !== iv) throw 'find';
const ser = coll.serializeInternal();
if (JSON.stringify(ser[0]) !== '{"end":6,"intervalType":2,"sequenceNumber":41,"start":2,"properties":{"referenceRangeLabels":["comments"],"author":"a"}}') throw 'serialize ' + JSON.stringify(ser[0]);
if (JSON.stringify(iv.serialize(client)) !== JSON.stringify(ser[0])) throw 'interval.serialize';
const order = [];
coll.map((x) => order.push(x.handle));
if (order.join() !== '0,1') throw 'map';
coll.delete(3, 3);
if (seen[2][0] !== 'delete' || seen[2][1] !== undefined || sent[1][0] !== 'delete') throw 'delete of nothing';
coll.deleteInterval({ start: 2, end: 6 }, false, { sequenceNumber: 51 });
if (seen[3][1] !== iv || seen[3][2] !== false || iv.handle !== undefined || sent.length !== 2 || des.length !== 3) throw 'remote delete';
if (coll.serializeInternal().length !== 1 || coll.findOverlappingIntervals(0, 7).length !== 0) throw 'after delete';
console.log('ok');
"""
    out = subprocess.run([NODE, '-e', src], cwd=REPO, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == 'ok', out.stderr
