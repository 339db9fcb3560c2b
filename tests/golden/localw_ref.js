"use strict";
// Fixture driver for the WIDE editing form (include/mtgpu.h "limits"): a farm of REFERENCE merge-tree
// Clients (the transpile under oracle/_tsref) behind a toy sequencer, logged as the editing client
// sees it -- the pattern of oracle/tsref/local_farm.js, with content past the narrow limits: text of
// Latin-1, BMP CJK and surrogate pairs (positions are code units: edits land between the halves of a
// pair), property keys 0..31, value ids up to 65535, markers that carry an id of their own (key
// MARKER_KEY, value ids from 256 up), and short client ids >= 64 and >= 256.
// TEST INFRASTRUCTURE ONLY (needs node and the transpile; tests/golden/make_localw.py runs it).
//
//   node localw_ref.js <kind> <seed> <nDocs> <edits>  -> one JSON line per kept document, then
//        {tried, kept, dropped}
//   kind: rounds | lag | promote | own_hi | reconnect | offline | long
//   document = {name, ids, records, states: [[k, state, text[, SnapshotV1 entries]], ...], regen, events,
//               counts, promote: {k, route, pending} | null, segs}
//   record = [seq, ref, msn, client, type, pos1, pos2, text, props {key id: value id | null} | null, flags]
//   (the editing client's local edits: seq -1; a reconnect's reset op: seq -2; oracle/tsref/replay_ref.js
//   documents the state and event forms, which are its own)
const path = require("path");
const ROOT = path.join(__dirname, "..", "..", "oracle", "_tsref", "merge-tree", "src");
const { Client } = require(path.join(ROOT, "client.js"));
const { TextSegment } = require(path.join(ROOT, "textSegment.js"));
const { Marker } = require(path.join(ROOT, "mergeTree.js"));
const { SnapshotV1 } = require(path.join(ROOT, "snapshotV1.js"));

const F_REWRITE = 1, F_GROUP_MORE = 4, F_MARKER = 128;
const MARKER_KEY = 7;
const logger = { send() {}, sendTelemetryEvent() {}, sendErrorEvent() {}, sendPerformanceEvent() {} };
function specToSegment(spec) { return TextSegment.fromJSONObject(spec) || Marker.fromJSONObject(spec); }

function rng(seed) {  // xorshift32
    let s = seed >>> 0 || 1;
    return () => {
        s ^= s << 13; s >>>= 0; s ^= s >>> 17; s ^= s << 5; s >>>= 0;
        return s / 4294967296;
    };
}

const kid = (k) => parseInt(k.slice(1), 10);
function propsOut(p) {
    if (!p) return null;
    const o = {};
    for (const k of Object.keys(p)) o[kid(k)] = p[k] === null || p[k] === undefined ? null : p[k];
    return o;
}
function record(seq, ref, msn, client, op) {
    if (op.type === 0) {
        const seg = op.seg;
        if (seg.marker) return [seq, ref, msn, client, 0, op.pos1, 0, String.fromCharCode(seg.marker.refType), propsOut(seg.props), F_MARKER];
        const text = typeof seg === "string" ? seg : seg.text;
        return [seq, ref, msn, client, 0, op.pos1, 0, text, typeof seg === "string" ? null : propsOut(seg.props), 0];
    }
    if (op.type === 1) return [seq, ref, msn, client, 1, op.pos1, op.pos2, null, null, 0];
    return [seq, ref, msn, client, 2, op.pos1, op.pos2, null, propsOut(op.props),
        op.combiningOp && op.combiningOp.name === "rewrite" ? F_REWRITE : 0];
}
function records(seq, ref, msn, client, op) {
    if (op.type !== 3) return [record(seq, ref, msn, client, op)];
    if (!op.ops.length) return [[seq, ref, msn, client, 3, 0, 0, null, null, 0]];
    return op.ops.map((m, i) => {
        const r = record(seq, ref, msn, client, m);
        if (i + 1 < op.ops.length) r[9] |= F_GROUP_MORE;
        return r;
    });
}
// what makes a record wide (oplog.py encode_record)
function wideRec(r) {
    const text = r[7] || "";
    for (let i = 0; i < text.length; i++) if (text.charCodeAt(i) > 255) return true;
    for (const k of Object.keys(r[8] || {})) if (parseInt(k, 10) >= 8 || (r[8][k] || 0) > 255) return true;
    return false;
}
const nonLatin = (t) => { for (let i = 0; i < (t || "").length; i++) if (t.charCodeAt(i) > 255) return true; return false; };

// ---- the canonical forms of oracle/tsref/replay_ref.js, restated (this file stands alone)
function logId(client, shortId) {
    if (shortId < 0) return -2;
    const long = client.getLongClientId(shortId);
    return long === "observer" ? 0 : parseInt(long.slice(1), 10);
}
const byKey = (a, b) => kid(a) - kid(b);
function leavesOf(c) {
    const out = [];
    const walk = (b) => {
        for (let i = 0; i < b.childCount; i++) {
            const ch = b.children[i];
            if (!ch.isLeaf()) walk(ch); else out.push(ch);
        }
    };
    walk(c.mergeTree.root);
    return out;
}
function canonical(client) {
    const mt = client.mergeTree;
    const segs = leavesOf(client).map((ch) => {
        const removed = ch.removedSeq !== undefined;
        const ov = (ch.removedClientOverlap || []).map((x) => logId(client, x)).sort((a, b) => a - b);
        let props = null;
        if (ch.properties) {
            props = {};
            for (const k of Object.keys(ch.properties).sort(byKey)) props[k] = ch.properties[k];
        }
        return [Marker.is(ch) ? { marker: ch.refType } : ch.text, ch.seq, logId(client, ch.clientId), removed ? ch.removedSeq : -1,
            removed ? logId(client, ch.removedClientId) : -1, ov, props];
    });
    const tree = [];
    let lvl = [mt.root];
    while (lvl.length) {
        tree.push(lvl.map((b) => b.childCount));
        const nxt = [];
        for (const b of lvl) for (let i = 0; i < b.childCount; i++) if (!b.children[i].isLeaf()) nxt.push(b.children[i]);
        lvl = nxt;
    }
    const w = mt.getCollabWindow();
    return { seq: w.currentSeq, msn: w.minSeq, segs, tree };
}
function attachEvents(c, seqRef, onAnnotate) {
    const events = [];
    const where = (seg) => {
        let ord = 0, pos = 0;
        for (const ch of leavesOf(c)) {
            if (ch.parent === undefined) continue;
            if (ch === seg) return [ord, pos];
            ord++;
            pos += ch.removedSeq === undefined ? ch.cachedLength : 0;
        }
        return [-1, -1];
    };
    const pdelta = (pd) => {
        if (!pd) return null;
        const o = {};
        for (const k of Object.keys(pd).sort(byKey)) o[k] = pd[k] === undefined ? null : pd[k];
        return o;
    };
    c.mergeTreeDeltaCallback = (opArgs, args) => {
        if (args.operation === 2 && seqRef.seq >= 0) onAnnotate(opArgs.op, args);
        events.push([seqRef.seq, args.operation, args.deltaSegments.map((d) => {
            const [leaf, pos] = where(d.segment);
            return [leaf, pos, d.segment.cachedLength, args.operation === 2 ? pdelta(d.propertyDeltas) : null];
        })]);
    };
    c.mergeTreeMaintenanceCallback = (args) => {
        const segs = [];
        for (let i = 0; i < args.deltaSegments.length; i++) {
            const seg = args.deltaSegments[i].segment;
            let leaf = where(seg)[0];
            if (args.operation === -2 && i === 1) leaf = segs[0][0] + 1;  // SPLIT: `next` not yet linked
            segs.push([leaf, -1, seg.cachedLength, null]);
        }
        events.push([seqRef.seq, args.operation, segs]);
    };
    return events;
}
function snapshotOf(c) {
    const snap = new SnapshotV1(c.mergeTree, logger);
    snap.extractSync();
    const entries = {};
    for (const e of snap.emit().entries) entries[e.path] = JSON.parse(e.value.contents);
    return entries;
}

// ---- the farm
// cfg: ids (short ids of the four clients, the editing client first), partial (the editing client
// lags), reconnect, offline, route (promote: 0 own wide local edit, 1 remote wide op, 2 remote id >= 64;
// the document stays narrow until `at` edits were made), quiet (the editing client's edits in all), cks (record counts to keep states at; none on
// the sizing pass), snap (a SnapshotV1 with each state)
function farm(seed, nOps, cfg) {
    const r = rng(seed);
    const ri = (n) => Math.floor(r() * n);
    const ids = cfg.ids, own = ids[0], nClients = ids.length;
    const clients = ids.map((id) => {
        const c = new Client(specToSegment, logger);
        c.startOrUpdateCollaboration("c" + id);
        return c;
    });
    const c1 = clients[0];
    const queue = [], seqd = [], cursor = clients.map(() => 0), log = [], regen = [], states = [];
    const counts = { wideLocal: 0, nonLatin: 0, key8: 0, key16: 0, rewrites: 0, overPending: 0, dropped: 0,
        pendingMax: 0, pendingAt: 0, regenOps: 0, regenWide: 0, local: 0 };
    const seqRef = { seq: 0 };
    // a remote annotate at the editing client (its ANNOTATE callback, before the counts change):
    // segments on which one of its keys >= 8 is pending locally, and segments whose pending local
    // rewrite drops it whole (propertyDeltas undefined)
    const events = attachEvents(c1, seqRef, (op, args) => {
        let over = false, drop = false;
        for (const d of args.deltaSegments) {
            const pm = d.segment.propertyManager;
            if (!pm) continue;
            if (pm.pendingRewriteCount > 0) drop = true;
            for (const k of Object.keys(op.props || {})) {
                if (kid(k) >= 8 && pm.pendingKeyUpdateCount && pm.pendingKeyUpdateCount[k] !== undefined) over = true;
            }
        }
        if (over) counts.overPending++;
        if (drop) counts.dropped++;
    });
    let seq = 0, made = 0, away = 0, nextMarker = 256, promote = null, wide = cfg.route === undefined;
    const text1 = (c) => c.createTextHelper().getText(c.getCurrentSeq(), c.getClientId());
    const want = (cfg.cks || []).slice();  // ascending record counts: the state at the first message end at or after each
    const pendingNow = () => c1.mergeTree.pendingSegments.count();
    const mark = () => {  // after every whole message / local edit of the editing client's log
        const k = log.length;
        if (want.length && k >= want[0]) {
            const st = [k, canonical(c1), text1(c1)];
            if (cfg.snap) st.push(snapshotOf(c1));
            states.push(st);
            while (want.length && want[0] <= k) want.shift();
        }
        if (pendingNow() > counts.pendingMax) {  // the most edits pending at once, and the record count there
            counts.pendingMax = pendingNow();
            counts.pendingAt = k;
        }
    };
    const push0 = (recs) => { log.push(...recs); mark(); };
    const deliver = (i) => {
        const m = seqd[cursor[i]++];
        if (i === 0) seqRef.seq = m.sequenceNumber;
        clients[i].applyMsg(m);
        if (i === 0) push0(records(m.sequenceNumber, m.referenceSequenceNumber, m.minimumSequenceNumber,
            parseInt(m.clientId.slice(1), 10), m.contents));
    };
    const ch = (w) => {  // one UTF-16 string piece
        const p = w ? r() : 0;
        if (p < 0.5) return String.fromCharCode(97 + ri(26));
        if (p < 0.6) return String.fromCharCode(0xC0 + ri(0x3F));             // Latin-1 upper half
        if (p < 0.85) return String.fromCharCode(0x4E00 + ri(0x5000));        // BMP CJK
        return String.fromCodePoint(0x1F600 + ri(64));                        // a surrogate pair
    };
    const keyOf = (w, hiRun) => {
        if (!w) return ri(4);
        if (hiRun) return 16 + ri(16);
        const p = r();
        return p < 0.35 ? ri(8) : p < 0.9 ? 8 + ri(3) : 11 + ri(21);
    };
    const valOf = (w) => (!w ? 1 + ri(200) : r() < 0.6 ? 1 + ri(255) : r() < 0.9 ? 256 + ri(4000) : 65535 - ri(3));
    const localOp = (i, forceWide) => {
        const c = clients[i];
        if (i === 0) seqRef.seq = -1;  // (a local edit's callbacks)
        const len = c.getLength();
        const w = wide || forceWide;
        const hiRun = w && (made % 97) >= 80;  // a run of edits on keys >= 16
        const pick = r();
        let op;
        if (len === 0 || pick < 0.42 || (forceWide && pick < 0.6)) {
            const n = 1 + ri(4);
            let text = "";
            for (let q = 0; q < n; q++) text += ch(w);
            if (forceWide) text += String.fromCharCode(0x4E00 + ri(0x5000));
            let props;
            if (r() < 0.25) { props = {}; props["k" + keyOf(w, hiRun)] = valOf(w); }
            let seg;
            if (w && !forceWide && r() < 0.12) {  // a marker with an id of its own
                seg = new Marker([1, 2, 4][ri(3)]);
                props = props || {};
                props["k" + MARKER_KEY] = nextMarker++;
            } else {
                seg = new TextSegment(text);
            }
            if (props) seg.addProperties(props);
            op = c.insertSegmentLocal(ri(len + 1), seg);
        } else {
            const a = ri(len), b = a + 1 + ri(Math.min(pick < 0.6 ? 6 : 14, len - a));
            if (pick < 0.6 && !forceWide) {
                op = c.removeRangeLocal(a, b);
            } else {
                const props = {};
                const nk = 1 + ri(w ? 3 : 2);
                for (let q = 0; q < nk; q++) props["k" + keyOf(w, hiRun)] = r() < 0.15 ? null : valOf(w);
                if (forceWide) props["k" + (8 + ri(8))] = valOf(true);
                op = c.annotateRangeLocal(a, b, props, r() < 0.1 ? { name: "rewrite" } : undefined);
            }
        }
        if (!op) throw new Error("local op rejected");
        queue.push({ client: i, ref: c.getCurrentSeq(), op, sg: c.peekPendingSegmentGroups() });
        if (i === 0) {
            counts.local++;
            const rec = record(-1, 0, 0, own, op);
            if (wideRec(rec)) {
                counts.wideLocal++;
                if (nonLatin(rec[7])) counts.nonLatin++;
                if (rec[4] === 2) {
                    const ks = Object.keys(rec[8]).map((k) => parseInt(k, 10));
                    if (ks.some((k) => k >= 8)) counts.key8++;
                    if (ks.some((k) => k >= 16)) counts.key16++;
                }
            }
            if (rec[4] === 2 && (rec[9] & F_REWRITE)) counts.rewrites++;
            push0([rec]);
        }
        made++;
        return op;
    };
    const sequenceAll = (hold) => {
        const held = [];
        while (queue.length) {
            const q = queue.shift();
            if (hold && q.client === 0) { held.push(q); continue; }
            seq++;
            const msn = Math.min(q.ref, ...clients.map((c) => c.getCurrentSeq()), ...queue.map((o) => o.ref),
                ...held.map((o) => o.ref));
            seqd.push({ clientId: "c" + ids[q.client], clientSequenceNumber: 1, contents: q.op, metadata: undefined,
                minimumSequenceNumber: msn, origin: undefined, referenceSequenceNumber: q.ref, sequenceNumber: seq,
                timestamp: 0, term: 1, traces: [], type: "op" });
        }
        queue.push(...held);
    };
    while (made < nOps) {
        if (cfg.offline && !away && r() < 0.08) away = 14 + ri(12);
        const promoting = !wide && made >= cfg.at;
        if (promoting) {
            // the promoting round: the editing client has edits pending when the document turns wide
            for (let q = 0; q < 2; q++) localOp(0, false);
            if (cfg.route === 0) {
                promote = { k: log.length, route: 0, pending: pendingNow() };
                localOp(0, true);
            } else {
                // a remote client's op -- wide (route 1), or by the client whose id is >= 64, silent
                // until now (route 2) -- sequenced and delivered while those edits are pending
                const held = queue.splice(0, queue.length);
                localOp(cfg.route === 1 ? 1 : nClients - 1, cfg.route === 1);
                sequenceAll(false);
                for (let i = 1; i < nClients; i++) while (cursor[i] < seqd.length) deliver(i);
                while (cursor[0] < seqd.length - 1) deliver(0);
                promote = { k: log.length, route: cfg.route, pending: pendingNow() };
                deliver(0);
                queue.push(...held);
            }
            wide = true;
        }
        for (let i = 0; i < nClients; i++) {
            if (!wide && cfg.route === 2 && i === nClients - 1) continue;  // (the id >= 64 stays silent)
            let k = away && i === 0 ? 2 + ri(5) : r() < 0.6 ? 1 + ri(3) : 0;
            // (quiet: the editing client makes cfg.quiet edits in all, spread over the run)
            if (cfg.quiet && i === 0) k = counts.local < cfg.quiet && made >= counts.local * (nOps / cfg.quiet) ? 1 : 0;
            for (let q = 0; q < k; q++) localOp(i, false);
        }
        let lost = [];
        if (cfg.reconnect && r() < 0.5) {
            lost = queue.filter((q) => q.client === 0);
            for (let q = queue.length - 1; q >= 0; q--) if (queue[q].client === 0) queue.splice(q, 1);
        }
        sequenceAll(away > 0);
        for (let i = 1; i < nClients; i++) while (cursor[i] < seqd.length) deliver(i);
        if (away) { away--; continue; }
        const upto = cfg.partial ? cursor[0] + ri(seqd.length - cursor[0] + 1) : seqd.length;
        while (cursor[0] < upto) deliver(0);
        for (const q of lost) {
            seqRef.seq = -2;
            const recs = records(-2, 0, 0, own, q.op);
            log.push(...recs);
            const op = c1.regeneratePendingOp(q.op, q.sg);
            const ops = (op.type === 3 ? op.ops : [op]).map((m) => record(0, 0, 0, own, m));
            counts.regenOps += ops.length;
            counts.regenWide += ops.filter(wideRec).length;
            regen.push([log.length - 1, ops.map((x) => x.slice(4))]);
            mark();
            queue.push({ client: 0, ref: c1.getCurrentSeq(), op, sg: undefined });
        }
        if (lost.length) {
            sequenceAll(false);
            for (let i = 0; i < nClients; i++) while (cursor[i] < seqd.length) deliver(i);
        }
    }
    sequenceAll(false);
    for (let i = 0; i < nClients; i++) while (cursor[i] < seqd.length) deliver(i);
    const t0 = text1(c1);
    for (const c of clients) if (text1(c) !== t0) return null;  // the reference's clients diverged: dropped
    if (pendingNow() !== 0) return null;
    states.push([log.length, canonical(c1), t0]);
    return { ids, records: log, states, regen, events, counts, promote, segs: leavesOf(c1).length };
}

const KINDS = {
    rounds: { ids: [1, 2, 70, 300] },
    lag: { ids: [1, 2, 70, 300], partial: true },
    promote: { ids: [1, 2, 3, 4], partial: true, at: 40 },
    own_hi: { ids: [70, 2, 3, 300], partial: true },
    reconnect: { ids: [1, 2, 70, 300], reconnect: true },
    offline: { ids: [1, 2, 70, 300], offline: true },
    // (few enough local edits that a launch of any size stays in the forms with one group-mask word)
    long: { ids: [1, 2, 70, 300], partial: true, quiet: 40 },
};

function main() {
    const [kind, seedS, nDocsS, nOpsS] = process.argv.slice(2);
    const seed = parseInt(seedS, 10), nDocs = parseInt(nDocsS, 10), nOps = parseInt(nOpsS, 10);
    let tried = 0, dropped = 0;
    const out = [];
    for (let d = 0; d < nDocs;) {
        const cfg = Object.assign({}, KINDS[kind]);
        if (kind === "promote") {
            cfg.route = Math.floor(d / 2);
            cfg.ids = cfg.route === 2 ? [1, 2, 3, 70] : [1, 2, 3, 4];
        }
        if (kind === "own_hi") cfg.ids = [[70, 2, 3, 300], [90, 2, 65, 3], [300, 2, 70, 3]][d % 3];
        const s = seed * 7919 + tried;
        tried++;
        let sized = null;
        try { sized = farm(s, nOps, cfg); } catch (e) { sized = null; }
        const ok = sized && (kind !== "promote" || (sized.promote && sized.promote.pending > 0)) &&
            (kind !== "offline" || sized.counts.pendingMax > 64) &&
            (kind === "long" || kind === "offline" || sized.records.length <= 400);
        if (!ok) { dropped++; continue; }
        // the second pass keeps the states: 5 checkpoints spread over the records (each moved to the
        // end of its message), the promoting record's two sides, the most edits pending
        const n = sized.records.length;
        const cks = new Set();
        for (let q = 1; q <= 5; q++) cks.add(Math.floor((q * n) / 6));
        if (kind === "offline") cks.add(sized.counts.pendingAt);
        if (sized.promote) {
            cks.clear();
            for (const q of [1, 4, 5]) cks.add(Math.floor((q * n) / 6));
            cks.add(sized.promote.k);
            cks.add(sized.promote.k + 1);
        }
        cfg.cks = [...cks].filter((k) => k > 0 && k < n).sort((a, b) => a - b);
        cfg.snap = kind === "lag" && d === 0;  // (SnapshotV1 at its checkpoints: pending edits elided)
        const doc = farm(s, nOps, cfg);
        doc.name = `${kind}_${d}`;
        out.push(doc);
        d++;
    }
    for (const doc of out) process.stdout.write(JSON.stringify(doc) + "\n");
    process.stdout.write(JSON.stringify({ tried, kept: out.length, dropped }) + "\n");
}
main();
