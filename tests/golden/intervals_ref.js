"use strict";
// Interval collections on the REFERENCE (the transpile under oracle/_tsref, intervalCollection.ts
// included by make_intervals.py): replays documents of a committed log on a reference Client -- the
// editing client "c<own>" of a local_* log, else the observer -- with a SequenceInterval collection
// attached (SequenceIntervalCollectionValueType.factory.load + attachGraph), and follows a plan
// (make_intervals.py) of queries, deletes and adds at message boundaries.
//
//   node intervals_ref.js <log.mtlog> <plan.json>   -> JSON lines, one per planned document:
//     {doc, err, steps: [{k, check, ops}], counts}
//   plan.json: {"<doc>": [{k, q: [{kind, u, v}], del: [{u}], add: [{u, v, mode, type}]}, ...]}
// A step runs after the message that ends at record count k (0: before the first), in this order, and
// records what it EXECUTED:
//   check  [[id, start ordinal | -1, start raw offset, start toPosition(), end ordinal | -1, end raw
//          offset, end toPosition()], ...] for every live interval, oldest first (ordinal: the segment's
//          index among the linked leaves; -1 without a segment or on an unlinked one)
//   ops    ["q", s, e, ids, tree, [ordinal | -1, offset], [ordinal | -1, offset] (, unlinked ids)]
//            ids: the live intervals x with x.overlaps(transient) -- the per-interval answer;
//            tree: findOverlappingIntervals(s, e) -- the tree's answer; then the transient interval's two
//            ends; then, if any, the live intervals with an end on an unlinked segment
//          ["d", id, s, e]  delete(s, e) by interval id's current toPosition() pair: the first interval,
//            from the planned one on, with both ends attached and for which the tree's lookup and the
//            per-interval equality search name the same single interval (each one passed over for
//            that is a skipped delete)
//          ["a", id, s, e, type]  add(s, e, type); skipped where it would duplicate a live interval
//            (compare-equal) or an end sits on an offset whose refsByOffset entry has no `at` list
//            (where addLocalRef throws, localReference.ts:212-219)
// counts: queries, tree_exact, skipped adds / deletes, how the intervals' ends moved, unlinked pairs.
const fs = require("fs");
const path = require("path");

const TS = path.join(__dirname, "..", "..", "oracle", "_tsref");
const ROOT = path.join(TS, "merge-tree", "src");
const { Client } = require(path.join(ROOT, "client.js"));
const { TextSegment } = require(path.join(ROOT, "textSegment.js"));
const { Marker } = require(path.join(ROOT, "mergeTree.js"));
const { SequenceIntervalCollectionValueType } = require(path.join(TS, "sequence", "src", "intervalCollection.js"));
const { loadLog, messages } = require(path.join(__dirname, "..", "..", "js", "mtlog.js"));

const TRANSIENT = 4;  // IntervalType.Transient

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
    const coll = new SequenceIntervalCollectionValueType().factory.load({ emit() {} }, []);
    coll.attachGraph(c, "comments");
    const view = coll.view;
    const local = view.localCollection;
    const ivs = [];  // {id, iv, removed, seg: [start's, end's], as of the last callback}
    const counts = { queries: 0, tree_exact: 0, skipped_add_duplicate: 0, skipped_add_no_at: 0, skipped_delete: 0,
        slid: 0, detached_remove: 0, born_detached: 0, unlinked_pairs: 0, pairs: 0, max_live: 0, adds: 0, deletes: 0 };
    let lastAdded;
    view.on("addInterval", (interval) => { lastAdded = interval; });
    const live = () => ivs.filter((r) => !r.removed);
    const settle = () => { for (const r of live()) r.seg = [r.iv.start.segment, r.iv.end.segment]; };
    c.mergeTreeMaintenanceCallback = () => settle();
    c.mergeTreeDeltaCallback = (opArgs, args) => {
        if (args.operation === 1) {
            for (const x of args.deltaSegments) {
                for (const r of live()) {
                    [r.iv.start, r.iv.end].forEach((ref, j) => {
                        if (r.seg[j] !== x.segment) return;
                        if (ref.segment === undefined) counts.detached_remove++;
                        else if (ref.segment !== x.segment) counts.slid++;
                    });
                }
            }
        }
        settle();
    };
    const transient = (s, e) => local.helpers.create("transient", s, e, c, TRANSIENT);
    const unlinked = (ref) => ref.segment !== undefined && ref.segment.parent === undefined;
    const steps = [];
    const doStep = (st) => {
        const order = new Map(leaves(c).map((s, i) => [s, i]));
        const ord = (ref) => (ref.segment !== undefined && order.has(ref.segment) ? order.get(ref.segment) : -1);
        const check = live().map((r) => [r.id, ord(r.iv.start), r.iv.start.offset, r.iv.start.toPosition(),
            ord(r.iv.end), r.iv.end.offset, r.iv.end.toPosition()]);
        const ops = [];
        const len = c.getLength();
        for (const q of st.q || []) {
            let s, e;
            if (q.kind === "all") { s = 0; e = len; }
            else if (q.kind === "past") { s = 0; e = len + 1; }
            else if (q.kind === "point") { s = e = q.u % (len + 1); }
            else if (q.kind === "head") { s = 0; e = q.u % (len + 2); }
            else { s = q.u % (len + 1); e = Math.min(len + 1, s + q.v % 12); }
            const tr = transient(s, e);
            const ids = live().filter((r) => r.iv.overlaps(tr)).map((r) => r.id);
            const byIv = new Map(live().map((r) => [r.iv, r.id]));
            const tree = view.findOverlappingIntervals(s, e).map((iv) => byIv.get(iv)).sort((a, b) => a - b);
            if (tree.some((id) => id === undefined)) throw new Error("the tree holds a removed interval");
            const un = live().filter((r) => unlinked(r.iv.start) || unlinked(r.iv.end)).map((r) => r.id);
            counts.queries++;
            counts.pairs += live().length;
            counts.unlinked_pairs += un.length;
            if (JSON.stringify(tree) === JSON.stringify(ids)) counts.tree_exact++;
            const rec = ["q", s, e, ids, tree, [ord(tr.start), tr.start.offset], [ord(tr.end), tr.end.offset]];
            if (un.length) rec.push(un);
            ops.push(rec);
        }
        for (const q of st.del || []) {
            // the first deletable interval from the (u mod n)-th on, oldest first
            const cand = live();
            let done = false;
            for (let t = 0; t < cand.length && !done; t++) {
                const r = cand[(q.u + t) % cand.length];
                const s = r.iv.start.toPosition(), e = r.iv.end.toPosition();
                if (s < 0 || e < 0) continue;
                const tr = transient(s, e);
                const same = cand.filter((x) => x.iv.compare(tr) === 0);
                const node = local.intervalTree.intervals.get(tr);
                if (same.length !== 1 || same[0] !== r || !node || node.key !== r.iv) { counts.skipped_delete++; continue; }
                view.delete(s, e);
                let still = false;
                view.map((iv) => { if (iv === r.iv) still = true; });
                if (still) throw new Error("delete left the interval in the tree");
                r.removed = true;
                counts.deletes++;
                ops.push(["d", r.id, s, e]);
                done = true;
            }
        }
        for (const q of st.add || []) {
            const n = c.getLength();
            const s = n ? q.u % n : 0;
            const e = q.mode === 1 ? n : q.mode === 2 ? n + 1 : Math.min(n, s + q.v % 9);
            const tr = transient(s, e);
            if (live().some((x) => x.iv.compare(tr) === 0)) { counts.skipped_add_duplicate++; continue; }
            const noAt = [s, e].some((p) => {
                const so = c.getContainingSegment(p);
                if (!so || !so.segment || !so.segment.localRefs) return false;
                const at = so.segment.localRefs.refsByOffset[so.offset];
                return at !== undefined && at.at === undefined;
            });
            if (noAt) { counts.skipped_add_no_at++; continue; }
            lastAdded = undefined;
            view.add(s, e, q.type, undefined);
            if (!lastAdded) throw new Error("addInterval made no interval");
            const iv = lastAdded;
            if (iv.start.segment === undefined) counts.born_detached++;
            if (iv.end.segment === undefined) counts.born_detached++;
            ivs.push({ id: ivs.length, iv, removed: false, seg: [iv.start.segment, iv.end.segment] });
            counts.adds++;
            ops.push(["a", ivs.length - 1, s, e, q.type]);
        }
        counts.max_live = Math.max(counts.max_live, live().length);
        steps.push({ k: st.k, check, ops });
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
        err = String(e.stack || e.message || e);
    }
    return { doc: d, err, steps, counts };
}

const log = loadLog(process.argv[2]);
const plans = JSON.parse(fs.readFileSync(process.argv[3], "utf8"));
const out = [];
for (const d of Object.keys(plans).map((x) => parseInt(x, 10)).sort((a, b) => a - b)) out.push(JSON.stringify(runDoc(log, d, plans[d])));
process.stdout.write(out.join("\n") + "\n");
