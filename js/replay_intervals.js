"use strict";
// Interval collections through the Node surface: documents of a log replayed into BatchClients that
// follow the executed steps of tests/golden/intervals.expected.jsonl (make_intervals.py) through
// getIntervalCollection("comments") -- findOverlappingIntervals, delete, add at the plan's record counts,
// serializeInternal at every step -- one JSON line per document {doc, err, steps: [{check: [[id, start,
// end], ...], q: [[id, ...], ...]}], events: {add, delete}, labels}.
//   node replay_intervals.js <log.mtlog> <fixture.jsonl> <log name> <n docs>
const fs = require("fs");
const { BatchEngine, IntervalType } = require("./batchClient.js");
const { loadLog, messages } = require("./mtlog.js");

const log = loadLog(process.argv[2]);
const name = process.argv[4], nDocs = parseInt(process.argv[5], 10);
const rows = fs.readFileSync(process.argv[3], "utf8").split("\n").filter((x) => x).map((x) => JSON.parse(x))
    .filter((r) => r.log === name && r.doc < nDocs);
const eng = new BatchEngine({ maxDocs: rows.length, opsPerLaunch: 16, intervalsPerDoc: 256, refsPerDoc: 512 });
const out = [];
for (const row of rows) {
    const items = [...messages(log, row.doc)];
    const own = items.find((x) => x.local);
    const c = eng.createClient();
    c.startOrUpdateCollaboration(own ? "c" + own.client : "observer");
    const sent = [];
    const coll = c.getIntervalCollection("comments", { emit: (op, prev, params) => sent.push(op) });
    if (c.getIntervalCollection("comments") !== coll) throw new Error("one collection per label");
    const other = c.getIntervalCollection("highlights");
    const ids = new Map();  // SequenceInterval -> id
    const events = { add: 0, delete: 0 };
    let lastAdded, lastDeleted;
    coll.on("addInterval", (iv, local) => { if (local) events.add++; lastAdded = iv; });
    coll.on("deleteInterval", (iv, local) => { if (local) events.delete++; lastDeleted = iv; });
    const steps = [];
    let err = null, si = 0, labels = true;
    const step = (st) => {
        const ser = coll.serializeInternal();
        const byHandle = [];
        coll.map((iv) => byHandle.push(iv));
        if (ser.length !== ids.size || byHandle.length !== ids.size) throw new Error("serializeInternal: a live interval is missing");
        const check = byHandle.map((iv, i) => {
            if (ser[i].intervalType !== iv.intervalType || ser[i].sequenceNumber !== c.getCurrentSeq()) throw new Error("serialize");
            if (ser[i].start !== iv.start.toPosition() || ser[i].end !== iv.end.toPosition()) throw new Error("serialize: positions");
            return [ids.get(iv), ser[i].start, ser[i].end];
        }).sort((a, b) => a[0] - b[0]);
        const q = [];
        for (const op of st.ops) {
            if (op[0] === "q") {
                q.push(coll.findOverlappingIntervals(op[1], op[2]).map((iv) => ids.get(iv)).sort((a, b) => a - b));
                if (other.findOverlappingIntervals(op[1], op[2]).length > 1) throw new Error("the other label's collection answered");
            } else if (op[0] === "d") {
                lastDeleted = undefined;
                coll.delete(op[2], op[3]);
                if (!lastDeleted || ids.get(lastDeleted) !== op[1]) throw new Error(`delete(${op[2]}, ${op[3]}) removed ${lastDeleted && ids.get(lastDeleted)}, not ${op[1]}`);
                ids.delete(lastDeleted);
            } else {
                lastAdded = undefined;
                coll.add(op[2], op[3], op[4], { id: op[1] });
                const iv = lastAdded;
                if (!iv || iv.intervalType !== op[4] || iv.properties.id !== op[1]) throw new Error("add: the event's interval");
                const lab = JSON.stringify(["comments"]);
                labels = labels && JSON.stringify(iv.properties.referenceRangeLabels) === lab &&
                    JSON.stringify(iv.start.getProperties().referenceRangeLabels) === lab && iv.start.pairedRef === iv.end &&
                    iv.end.pairedRef === iv.start && ((iv.start.refType & 0x40) !== 0) === ((op[4] & IntervalType.SlideOnRemove) !== 0) &&
                    ((iv.start.refType & 0x2) !== 0) === (op[4] === IntervalType.Nest);
                ids.set(iv, op[1]);
            }
        }
        steps.push({ check, q });
    };
    try {
        // the other label's collection holds one interval of its own throughout: detached from birth on
        // the empty document, seen by no query of "comments"
        other.add(0, 1, 0, undefined);
        while (si < row.steps.length && row.steps[si].k === 0) step(row.steps[si++]);
        for (const it of items) {
            if (it.regen) {
                c.regeneratePendingOp(it.op);
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
            while (si < row.steps.length && row.steps[si].k === it.end) step(row.steps[si++]);
        }
        // a remote value-type op: no op is sent, the event says local === false
        const before = sent.length;
        let remote;
        coll.once("addInterval", (iv, local, op) => { remote = [iv, local, op]; });
        coll.addInternal({ start: 0, end: 0, intervalType: 0, sequenceNumber: 0 }, false, { sequenceNumber: 7 });
        if (!remote || remote[1] !== false || remote[2].sequenceNumber !== 7 || sent.length !== before) throw new Error("addInternal (remote)");
        if (sent.filter((x) => x === "add").length !== events.add || sent.filter((x) => x === "delete").length !== events.delete) throw new Error("emitter");
    } catch (e) {
        err = String(e.stack || e.message || e);
    }
    out.push(JSON.stringify({ doc: row.doc, err, steps, events, labels }));
}
process.stdout.write(out.join("\n") + "\n");
