"use strict";
// Marker-relative ops through the Node surface: documents of tests/golden/relpos*.mtlog replayed into
// BatchClients -- the observer's log through applyMsg, relative ops included; the editing client's log
// with its annotateMarker edits made through BatchClient.annotateMarker -- and, at the fixture's
// checkpoints (tests/golden/relpos.expected.jsonl), the canonical state and the posFromRelativePos
// answers; one JSON line per document
//   {doc, err, states: [[k, state]], pfr: [[k, answer, ...]], ops: <annotateMarker ops compared>}.
// States are BatchClient.getState()'s: long client ids, property keys and values by name ("k1": 3,
// "markerId": "m7") -- the host interns them in its own order.
//   node replay_relpos.js <log.mtlog> <fixture.jsonl> <log name> <markerKey>
const fs = require("fs");
const { BatchEngine } = require("./batchClient.js");
const { loadLog, messages } = require("./mtlog.js");

const log = loadLog(process.argv[2]);
const name = process.argv[4], opts = { markerKey: parseInt(process.argv[5], 10) };
const rows = fs.readFileSync(process.argv[3], "utf8").split("\n").filter((x) => x).map((x) => JSON.parse(x))
    .filter((r) => r.log === name);
const eng = new BatchEngine({ maxDocs: rows.length, opsPerLaunch: 16 });
const sorted = (v) => (v && typeof v === "object" && !Array.isArray(v)
    ? Object.keys(v).sort().reduce((o, k) => { o[k] = sorted(v[k]); return o; }, {}) : v);
const same = (a, b) => JSON.stringify(sorted(a)) === JSON.stringify(sorted(b));
const out = [];
for (const row of rows) {
    const items = [...messages(log, row.doc, opts)];
    const own = items.find((x) => x.local);
    const c = eng.createClient();
    c.startOrUpdateCollaboration(own ? "c" + own.client : "observer");
    // the editing client's edits are acked in order: edit j's ack is its j-th own sequenced message, and a
    // relative ack says the edit was an annotateMarker of that id
    const acks = own ? items.filter((x) => !x.local && !x.regen && x.clientId === "c" + own.client) : [];
    const states = [], pfr = [];
    let err = null, nLocal = 0, compared = 0;
    const checkpoint = (k) => {
        if (!row.checkpoints.some((x) => x.k === k)) return;
        states.push([k, c.getState()]);
        for (const q of row.pfr.filter((x) => x[0] === k)) {
            const rel = { id: "m" + q[2], before: q[3] };
            if (q[4] !== null) rel.offset = q[4];
            pfr.push(q[1] === null ? c.posFromRelativePos(rel) : c.posFromRelativePos(rel, q[1][0], c._shortId("c" + q[1][1])));
        }
    };
    try {
        for (const it of items) {
            if (it.local) {
                const ack = acks[nLocal++], op = it.op;
                if (ack && ack.contents.relativePos1) {
                    const marker = c.getMarkerFromId(ack.contents.relativePos1.id);
                    const sent = c.annotateMarker(marker, op.props, op.combiningOp);
                    if (!same(sent, ack.contents)) throw new Error(`annotateMarker: ${JSON.stringify(sent)} != ${JSON.stringify(ack.contents)}`);
                    compared++;
                } else if (op.type === 0) {
                    if (op.seg.marker) c.insertMarkerLocal(op.pos1, op.seg.marker.refType, op.seg.props);
                    else c.insertTextLocal(op.pos1, typeof op.seg === "string" ? op.seg : op.seg.text, op.seg.props);
                } else if (op.type === 1) c.removeRangeLocal(op.pos1, op.pos2);
                else c.annotateRangeLocal(op.pos1, op.pos2, op.props, op.combiningOp);
            } else {
                c.applyMsg(it);
            }
            checkpoint(it.end);
        }
    } catch (e) {
        err = String(e.stack || e.message || e);
    }
    out.push(JSON.stringify({ doc: row.doc, err, states, pfr, ops: compared }));
}
process.stdout.write(out.join("\n") + "\n");
