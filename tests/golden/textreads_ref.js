"use strict";
// Text reads on the REFERENCE (the transpile under oracle/_tsref): replays documents of a committed log
// on a reference Client -- the editing client "c<own>" of a local_* log, else the observer -- and, at
// message boundaries, follows a plan (make_textreads.py) of createTextHelper().getText /
// getTextAndMarkers calls.
//
//   node textreads_ref.js <log.mtlog> <plan.json> [tileKey]  -> JSON lines, one per planned document:
//     {doc, err, steps: [{k, ops}], counts}
//   plan.json: {"<doc>": [{k, reads: [{kind, u, v, ph | label, remote}], ...}, ...]}
// A step runs after the message that ends at record count k (0: before the first) and records what it
// EXECUTED, inputs then outputs:
//   ["t", view, placeholder, start | null, end | null, text (, [marker.toString(), ...])]
//        getText(refSeq, clientId, placeholder, start, end); with the "*" placeholder also the
//        toString() of every marker the same mapRange visits, in order
//   ["m", view, label, start | null, end | null, parallelText, [marker ordinal, ...]]
//        getTextAndMarkers(refSeq, clientId, label, start, end); a marker's ordinal is its index among
//        the linked leaves
// view: null -- the client's own (currentSeq, its own short id) -- or [refSeq, c] for the view of the
// log's client c at refSeq (its latest op's own pair, not below minSeq; observer documents only).  null start / end: undefined.
// counts: reads by kind, start > end reads with non-empty text, reads with edits pending, ...
const fs = require("fs");
const path = require("path");

const TS = path.join(__dirname, "..", "..", "oracle", "_tsref");
const ROOT = path.join(TS, "merge-tree", "src");
const { Client } = require(path.join(ROOT, "client.js"));
const { TextSegment } = require(path.join(ROOT, "textSegment.js"));
const { Marker } = require(path.join(ROOT, "mergeTree.js"));
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

function runDoc(log, d, plan, opts) {
    const items = [...messages(log, d, opts)];
    const own = items.find((x) => x.local);
    const logger = { send() {}, sendTelemetryEvent() {}, sendErrorEvent() {}, sendPerformanceEvent() {} };
    const c = new Client(specToSegment, logger);
    c.startOrUpdateCollaboration(own ? "c" + own.client : "observer");
    const helper = c.createTextHelper();
    const counts = { reads: 0, all: 0, viewport: 0, point: 0, neg: 0, past: 0, swap: 0, swap_nonempty: 0, endle0: 0,
        star: 0, star_markers: 0, space_markers: 0, tm: 0, tm_cuts: 0, tm_absent: 0, remote: 0, remote_differs: 0,
        pending: 0, units: 0 };
    // each remote client's view as of its latest message: [refSeq, client].  An older pair of the same
    // client is no view any more: the client has since acted on what it had seen by its later refSeq,
    // and the reference's partial lengths (the default `end`, the blocks' lengths) count that.
    const seen = new Map();
    const steps = [];
    const doStep = (st) => {
        const ops = [];
        const pending = c.mergeTree.pendingSegments !== undefined && !c.mergeTree.pendingSegments.empty();
        for (const q of st.reads) {
            // the view
            let refSeq = c.getCurrentSeq(), clientId = c.getClientId(), view = null;
            if (q.remote && !own) {
                const minSeq = c.getCollabWindow().minSeq;
                const ok = [...seen.values()].filter((x) => x[0] >= minSeq).sort((a, b) => a[1] - b[1]);
                if (ok.length) {
                    view = ok[q.remote % ok.length];
                    refSeq = view[0];
                    clientId = c.getOrAddShortClientId("c" + view[1]);
                }
            }
            const len = c.mergeTree.getLength(refSeq, clientId);
            let s, e;
            if (q.kind === "all") { s = undefined; e = undefined; }
            else if (q.kind === "viewport") { s = q.u % (len + 1); e = s + 1 + q.v % 80; }
            else if (q.kind === "point") { s = e = q.u % (len + 1); }
            else if (q.kind === "neg") { s = -1 - q.u % 5; e = q.v % (len + 2); }
            else if (q.kind === "past") { s = q.u % (len + 1); e = len + 1 + q.v % 7; }
            else if (q.kind === "endle0") { s = -(q.u % 3); e = -(q.v % 3); }
            else if (q.kind === "swap") {
                // start > end inside one segment of the view at least three units long, if there is one
                const cand = [];
                let p = 0;
                for (const seg of leaves(c)) {
                    const l = c.mergeTree.nodeLength(seg, refSeq, clientId);
                    if (l >= 3 && TextSegment.is(seg)) cand.push([p, l]);
                    p += l;
                }
                if (cand.length) {
                    const [p0, l] = cand[q.u % cand.length];
                    const a = 2 + q.v % (l - 2), b = 1 + (q.u >> 8) % (a - 1);
                    s = p0 + a; e = p0 + b;
                } else { s = Math.min(len, 1 + q.u % (len + 1)); e = s - 1; }
            } else throw new Error("plan: unknown kind " + q.kind);
            const rs = s === undefined ? null : s, re = e === undefined ? null : e;
            counts.reads++;
            counts[q.kind]++;
            if (pending) counts.pending++;
            if (view) {
                counts.remote++;
                if (len !== c.getLength()) counts.remote_differs++;
            }
            if (q.label !== undefined) {
                const order = new Map(leaves(c).map((x, i) => [x, i]));
                const r = helper.getTextAndMarkers(refSeq, clientId, q.label, s, e);
                const ords = r.parallelMarkers.map((m) => order.get(m));
                if (ords.some((o) => o === undefined)) throw new Error("a marker outside the linked leaves");
                counts.tm++;
                counts.tm_cuts += ords.length;
                if (!ords.length) counts.tm_absent++;
                ops.push(["m", view, q.label, rs, re, r.parallelText, ords]);
                continue;
            }
            const text = helper.getText(refSeq, clientId, q.ph, s, e);
            counts.units += text.length;
            if (q.kind === "swap" && s > e && text.length > 0) counts.swap_nonempty++;
            const rec = ["t", view, q.ph, rs, re, text];
            const strings = [];
            c.mergeTree.mapRange({ leaf: (seg) => { if (!TextSegment.is(seg)) strings.push(seg.toString()); return true; } },
                refSeq, clientId, undefined, s === undefined ? 0 : s, e === undefined ? len : e);
            if (q.ph === "*") {
                counts.star++;
                counts.star_markers += strings.length;
                rec.push(strings);
            } else if (q.ph === " ") {
                counts.space_markers += strings.length;
            }
            ops.push(rec);
        }
        steps.push({ k: st.k, ops });
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
                if (it.contents) {
                    const cl = parseInt(it.clientId.slice(1), 10);
                    seen.set(cl, [it.referenceSequenceNumber, cl]);
                }
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
const opts = process.argv[4] !== undefined ? { tileKey: parseInt(process.argv[4], 10) } : undefined;
const out = [];
for (const d of Object.keys(plans).map((x) => parseInt(x, 10)).sort((a, b) => a - b)) out.push(JSON.stringify(runDoc(log, d, plans[d], opts)));
process.stdout.write(out.join("\n") + "\n");
