"use strict";
// Local references on the REFERENCE merge-tree (the transpile under oracle/_tsref): replays documents
// of a committed log on a reference Client -- the editing client "c<own>" of a local_* log, else the
// observer -- and follows a plan (make_localrefs.py) of LocalReference adds / removes / checkpoints.
//
//   node localrefs_ref.js <log.mtlog> <plan.json>   -> JSON lines, one per planned document:
//     {doc, err, steps: [{k, check, remove, add}], counts}
//   plan.json: {"<doc>": [{k, remove: [{id} | {u}], add: [{pos, type} | {u, type}]}, ...]}
// A step runs after the message that ends at record count k (0: before the first), in the order
//   check   [[id, toPosition(), ordinal | -1, getOffset()], ...] for every reference ever added and not
//           removed by the plan (ordinal: the segment's index among the linked leaves; a reference
//           whose segment is undefined has no getOffset(): 0)
//   remove  [id, ...]: removeLocalReference ({u}: the (u mod n)-th of the n live references that still
//           have a segment, oldest first -- the reference throws on one without; none if n is 0)
//   add     [[id, pos, type], ...]: new LocalReference(client, seg, off, type) + addLocalReference at
//           getContainingSegment(pos) ({u}: pos = u mod length; skipped on an empty document)
// counts: how the references moved, by the reference's own four movers (observed in its callbacks).
const fs = require("fs");
const path = require("path");

const ROOT = path.join(__dirname, "..", "..", "oracle", "_tsref", "merge-tree", "src");
const { Client } = require(path.join(ROOT, "client.js"));
const { TextSegment } = require(path.join(ROOT, "textSegment.js"));
const { Marker } = require(path.join(ROOT, "mergeTree.js"));
const { LocalReference } = require(path.join(ROOT, "localReference.js"));
const { loadLog, messages } = require(path.join(__dirname, "..", "..", "js", "mtlog.js"));

function specToSegment(spec) { return TextSegment.fromJSONObject(spec) || Marker.fromJSONObject(spec); }

function leaves(c) {
    const out = [];
    const walk = (b) => {
        for (let i = 0; i < b.childCount; i++) {
            const ch = b.children[i];
            if (!ch.isLeaf()) walk(ch); else if (ch.parent !== undefined) out.push(ch);
        }
    };
    walk(c.mergeTree.root);
    return out;
}

function runDoc(log, d, plan) {
    const items = [...messages(log, d)];
    const own = items.find((x) => x.local);
    const logger = { send() {}, sendTelemetryEvent() {}, sendErrorEvent() {}, sendPerformanceEvent() {} };
    const c = new Client(specToSegment, logger);
    c.startOrUpdateCollaboration(own ? "c" + own.client : "observer");
    const refs = [];  // {id, ref, removed, seg, off}: seg / off as of the last callback
    const counts = { split: 0, append: 0, slid_before: 0, slid_after: 0, detached_remove: 0, detached_unlink: 0,
        kept_by_clear: 0 };
    const live = () => refs.filter((r) => !r.removed);
    const settle = () => { for (const r of live()) { r.seg = r.ref.segment; r.off = r.ref.offset; } };
    c.mergeTreeMaintenanceCallback = (args) => {
        const segs = args.deltaSegments.map((x) => x.segment);
        for (const r of live()) {
            if (args.operation === -2 && r.seg === segs[0] && r.ref.segment === segs[1]) counts.split++;
            if (args.operation === -1 && r.seg === segs[1] && r.ref.segment === segs[0]) counts.append++;
            if (args.operation === -3 && r.ref.segment === segs[0] && !r.unlinked) { r.unlinked = true; counts.detached_unlink++; }
        }
        settle();
    };
    c.mergeTreeDeltaCallback = (opArgs, args) => {
        if (args.operation === 1) {
            const order = leaves(c);
            for (const x of args.deltaSegments) {
                for (const r of live()) {
                    if (r.seg !== x.segment) continue;
                    if (r.ref.segment === undefined) counts.detached_remove++;
                    else if (r.ref.segment === x.segment) counts.kept_by_clear++;
                    else if (order.indexOf(r.ref.segment) > order.indexOf(x.segment)) counts.slid_before++;
                    else counts.slid_after++;
                }
            }
        }
        settle();
    };
    const steps = [];
    const doStep = (st) => {
        const order = leaves(c);
        const check = live().map((r) => [r.id, r.ref.toPosition(), r.ref.segment ? order.indexOf(r.ref.segment) : -1,
            r.ref.segment ? r.ref.getOffset() : 0]);
        const removed = [];
        for (const q of st.remove || []) {
            let r;
            if (q.id !== undefined) {
                r = refs[q.id];
            } else {
                const cand = live().filter((x) => x.ref.segment !== undefined);
                if (cand.length) r = cand[q.u % cand.length];
            }
            if (!r || r.removed) continue;
            c.removeLocalReference(r.ref);
            r.removed = true;
            removed.push(r.id);
        }
        const added = [], throws = [];
        for (const q of st.add || []) {
            const len = c.getLength();
            if (q.pos === undefined && len === 0) continue;
            const pos = q.pos !== undefined ? q.pos : q.u % len;
            const so = c.getContainingSegment(pos);
            if (!so.segment) throw new Error(`plan: no segment at ${pos}`);
            const ref = new LocalReference(c, so.segment, so.offset, q.type);
            try {
                c.addLocalReference(ref);
            } catch (e) {
                // addLocalRef pushes onto refsByOffset[offset].at, which a slide creates without an `at`
                // list (localReference.ts:212-219, 323-326): the add throws before it changes anything
                if (!(e instanceof TypeError)) throw e;
                throws.push([pos, q.type]);
                continue;
            }
            refs.push({ id: refs.length, ref, removed: false, seg: so.segment, off: so.offset });
            added.push([refs.length - 1, pos, q.type]);
        }
        steps.push(throws.length ? { k: st.k, check, remove: removed, add: added, add_throws: throws }
            : { k: st.k, check, remove: removed, add: added });
    };
    let err = null, si = 0;
    try {
        while (si < plan.length && plan[si].k === 0) doStep(plan[si++]);
        for (const it of items) {
            if (it.regen) {
                c.regeneratePendingOp(it.op, c.mergeTree.pendingSegments.first());
            } else if (it.local) {
                const op = it.op;
                if (op.type === 0) c.insertSegmentLocal(op.pos1, specToSegment(op.seg));
                else if (op.type === 1) c.removeRangeLocal(op.pos1, op.pos2);
                else c.annotateRangeLocal(op.pos1, op.pos2, op.props, op.combiningOp);
            } else {
                c.applyMsg(it);
            }
            while (si < plan.length && plan[si].k === it.end) doStep(plan[si++]);
        }
        if (si !== plan.length) throw new Error(`plan: step at k=${plan[si].k} is not a message boundary`);
    } catch (e) {
        err = String(e.message || e);
    }
    return { doc: d, err, steps, counts };
}

const log = loadLog(process.argv[2]);
const plans = JSON.parse(fs.readFileSync(process.argv[3], "utf8"));
const out = [];
for (const d of Object.keys(plans).map((x) => parseInt(x, 10)).sort((a, b) => a - b)) out.push(JSON.stringify(runDoc(log, d, plans[d])));
process.stdout.write(out.join("\n") + "\n");
