"use strict";
// Local references through the Node surface: documents of a log replayed into BatchClients that follow
// the plan of tests/golden/localrefs.expected.jsonl (make_localrefs.py) -- createLocalReference /
// removeLocalReference at the plan's record counts, toPosition() / getSegment() / getOffset() of every
// reference at every step -- one JSON line per document {doc, err, steps: [[[id, position, ordinal,
// offset], ...], ...]}.
//   node replay_localrefs.js <log.mtlog> <fixture.jsonl> <log name> <n docs> [sync]
const fs = require("fs");
const { BatchEngine } = require("./batchClient.js");
const { loadLog, messages } = require("./mtlog.js");

const log = loadLog(process.argv[2]);
const name = process.argv[4], nDocs = parseInt(process.argv[5], 10);
const rows = fs.readFileSync(process.argv[3], "utf8").split("\n").filter((x) => x).map((x) => JSON.parse(x))
    .filter((r) => r.log === name && r.doc < nDocs);
const eng = new BatchEngine({ maxDocs: rows.length, opsPerLaunch: 16, syncCallbacks: process.argv[6] === "sync" });
const out = [];
for (const row of rows) {
    const items = [...messages(log, row.doc)];
    const own = items.find((x) => x.local);
    const c = eng.createClient();
    c.startOrUpdateCollaboration(own ? "c" + own.client : "observer");
    if (process.argv[6] === "sync") c.mergeTreeDeltaCallback = () => {};  // (per-message flushes)
    const refs = new Map(), steps = [];
    let err = null, si = 0;
    const step = (st) => {
        const check = [];
        for (const [id, ref] of refs) {
            const seg = ref.getSegment();
            const pos = ref.toPosition();
            if (c.referencePositionToLocalPosition(ref) !== pos) throw new Error("referencePositionToLocalPosition");
            check.push([id, pos, seg ? seg.ordinal : -1, ref.getOffset()]);
        }
        steps.push(check);
        for (const id of st.remove) { c.removeLocalReference(refs.get(id)); refs.delete(id); }
        for (const [id, pos, type] of st.add) refs.set(id, c.createLocalReference(pos, type));
    };
    try {
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
        // compare / min / max: document order, a detached reference first
        const all = [...refs.values()];
        for (let i = 0; i + 1 < all.length; i++) {
            const a = all[i], b = all[i + 1];
            const pa = a.toPosition(), pb = b.toPosition();
            const cmp = a.compare(b);
            if (pa >= 0 && pb >= 0 && pa !== pb && (cmp < 0) !== (pa < pb)) throw new Error("compare disagrees with toPosition");
            if (pa < 0 && pb >= 0 && cmp >= 0) throw new Error("a detached reference does not sort first");
            if (a.min(b) !== (cmp < 0 ? a : b) || a.max(b) !== (cmp > 0 ? a : b)) throw new Error("min / max");
        }
        if (all.length) {
            all[0].addProperties({ k: 1, gone: 2 });
            all[0].addProperties({ gone: null });
            if (JSON.stringify(all[0].getProperties()) !== "{\"k\":1}" || all[0].isLeaf()) throw new Error("properties");
        }
    } catch (e) {
        err = String(e.message || e);
    }
    out.push(JSON.stringify({ doc: row.doc, err, steps }));
}
process.stdout.write(out.join("\n") + "\n");
