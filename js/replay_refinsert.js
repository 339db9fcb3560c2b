"use strict";
// insertAtReferencePositionLocal through the Node surface: the documents of a refinsert log
// (tests/golden/refinsert*.mtlog) replayed into editing BatchClients that add the fixture's references
// (tests/golden/refinsert.expected.jsonl `refs`) and make every type-5 record through
// BatchClient.insertAtReferencePositionLocal -- one JSON line per document
//   {doc, err, ats: [{op: pos1 | null, cbs: [[operation, [[ordinal, position, cachedLength], ...], local], ...]}], state}
// cbs: the delta callbacks fired inside the call (local: opArgs carries the op and no sequencedMessage).
//   node replay_refinsert.js <log.mtlog> <fixture.jsonl> <log name> <marker key>
const fs = require("fs");
const { BatchEngine } = require("./batchClient.js");
const { loadLog, messages } = require("./mtlog.js");

const log = loadLog(process.argv[2]);
const name = process.argv[4], markerKey = parseInt(process.argv[5], 10);
const rows = fs.readFileSync(process.argv[3], "utf8").split("\n").filter((x) => x).map((x) => JSON.parse(x))
    .filter((r) => r.log === name);
const eng = new BatchEngine({ maxDocs: rows.length, opsPerLaunch: 16, refsPerDoc: 32 });
const out = [];
for (const row of rows) {
    const c = eng.createClient();
    c.startOrUpdateCollaboration("c1");
    let cbs = null;
    c.mergeTreeDeltaCallback = (opArgs, args) => {
        if (cbs) {
            cbs.push([args.operation, args.deltaSegments.map((x) => [x.segment.ordinal, x.segment.position, x.segment.cachedLength]),
                opArgs !== undefined && opArgs.op !== undefined && opArgs.sequencedMessage === undefined]);
        }
    };
    const refs = [], ats = [];
    const plan = row.refs.slice();
    let err = null;
    try {
        for (const it of messages(log, row.doc, { markerKey })) {
            while (plan.length && plan[0][0] === it.end - 1) {
                const [, id, pos, type] = plan.shift();
                if (id !== refs.length) throw new Error("plan: reference ids are not in order");
                refs.push(c.createLocalReference(pos, type));
            }
            if (it.local && it.op.refId !== undefined) {
                eng.flush();
                cbs = [];
                const op = c.insertAtReferencePositionLocal(refs[it.op.refId], it.op.seg);
                if (op && (op.type !== 0 || JSON.stringify(op.seg) !== JSON.stringify(it.op.seg))) throw new Error("the returned op's segment");
                ats.push({ op: op ? op.pos1 : null, cbs });
                cbs = null;
            } else if (it.local) {
                const op = it.op;
                if (op.type === 0) {
                    if (typeof op.seg === "string") c.insertTextLocal(op.pos1, op.seg);
                    else if (op.seg.marker) c.insertMarkerLocal(op.pos1, op.seg.marker.refType, op.seg.props);
                    else c.insertTextLocal(op.pos1, op.seg.text, op.seg.props);
                } else if (op.type === 1) {
                    c.removeRangeLocal(op.pos1, op.pos2);
                } else {
                    c.annotateRangeLocal(op.pos1, op.pos2, op.props, op.combiningOp);
                }
            } else {
                c.applyMsg(it);
            }
        }
        for (const [, , pos, type] of plan) refs.push(c.createLocalReference(pos, type));  // (after the last record)
    } catch (e) {
        err = String(e.stack || e);
    }
    let state = null;
    try { state = c.getState(); } catch (e) { err = err || String(e.stack || e); }
    out.push(JSON.stringify({ doc: row.doc, err, ats, state }));
}
process.stdout.write(out.join("\n") + "\n");
