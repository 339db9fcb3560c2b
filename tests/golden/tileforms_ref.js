"use strict";
// Fixture driver for findTile / getStackContext in every form of the apply engine: a farm of REFERENCE
// merge-tree Clients (the transpile under oracle/_tsref) behind a toy sequencer, logged as ONE client sees
// it -- the pattern of tests/golden/localw_ref.js and oracle/tsref/local_farm.js -- with about a third of
// the inserts markers (Tile, NestBegin, NestEnd) that carry real referenceTileLabels / referenceRangeLabels
// arrays over L0..L3, and annotates (plain, rewrite, null) that change those labels.  At message
// boundaries the logged client is asked findTile(p, "L"+l, preceding) and getStackContext(p, ["L"+l]);
// beside each answer goes the PLAIN answer: a flat walk over the client's leaves with their current
// labels (the answer a merge tree without block caches would give).
// TEST INFRASTRUCTURE ONLY (needs node and the transpile; tests/golden/make_tileforms.py runs it).
//
//   node tileforms_ref.js <kind> <seed> <nDocs> <edits>  -> one JSON line per kept document, then
//        {tried, kept, dropped}
//   kind: scenarios | edit | edit_lag | edit_reconnect | edit_offline | wide | edit_wide
//   document = {name, ids, observer, keys: [tile key, range key], records, checkpoints, counts, promote, segs}
//   record = [seq, ref, msn, client, type, pos1, pos2, text, props {key id: value id | null} | null, flags]
//     (the logged client's local edits: seq -1; a reconnect's reset op: seq -2); a label array is logged
//     as the bitmask of its labels (js/mtlog.js tileLabels) under the document's tile / range key
//   checkpoint = {k, len, why, pend: [edits pending, label annotates pending], removed, pos: [p, ...],
//                 tiles: [reference, plain], stacks: [reference, plain], ptile}
//     after k records; tiles: per p, per l in 0..3, preceding then not: the tile's position | -1;
//     stacks: per p, per l: [[marker position, refType], ...] bottom to top; why: "ann" (the record before
//     is a label annotate), "pre" / "ack" (before / after a message that is the ack of the logged client's
//     own label annotate), "spread", "end"; removed: tiles locally removed and unacked; ptile: answers
//     naming a tile the logged client inserted and that is not acked
const path = require("path");
const ROOT = path.join(__dirname, "..", "..", "oracle", "_tsref", "merge-tree", "src");
const { Client } = require(path.join(ROOT, "client.js"));
const { TextSegment } = require(path.join(ROOT, "textSegment.js"));
const { Marker } = require(path.join(ROOT, "mergeTree.js"));

const F_REWRITE = 1, F_GROUP_MORE = 4, F_MARKER = 128;
const TILE = 1, NEST_BEGIN = 2, NEST_END = 4;
const TL = "referenceTileLabels", RL = "referenceRangeLabels";
const MAX_POS = 24;
const logger = { send() {}, sendTelemetryEvent() {}, sendErrorEvent() {}, sendPerformanceEvent() {} };
function specToSegment(spec) { return TextSegment.fromJSONObject(spec) || Marker.fromJSONObject(spec); }

function rng(seed) {  // xorshift32
    let s = seed >>> 0 || 1;
    return () => {
        s ^= s << 13; s >>>= 0; s ^= s >>> 17; s ^= s << 5; s >>>= 0;
        return s / 4294967296;
    };
}

const labelsOf = (mask) => [0, 1, 2, 3].filter((i) => (mask >> i) & 1).map((i) => "L" + i);
const maskOf = (arr) => arr.reduce((m, l) => m | (1 << parseInt(l.slice(1), 10)), 0);

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
// a leaf's length in its client's own view
const localLen = (s) => (s.removedSeq === undefined ? s.cachedLength : 0);

// ---- the plain answers: flat walks with the leaves' current labels
const isTile = (s, label) => Marker.is(s) && (s.refType & TILE) !== 0 && !!s.properties &&
    Array.isArray(s.properties[TL]) && s.properties[TL].includes(label);
const isRange = (s, label) => Marker.is(s) && (s.refType & (NEST_BEGIN | NEST_END)) !== 0 && !!s.properties &&
    Array.isArray(s.properties[RL]) && s.properties[RL].includes(label);
const posOf = (lv, seg) => {
    let at = 0;
    for (const s of lv) {
        if (s === seg) return at;
        at += localLen(s);
    }
    throw new Error("a segment outside the leaves");
};
function plainTile(lv, pos, label, preceding) {
    let tile;
    if (preceding) {
        let p = pos;
        for (const s of lv) {
            const len = localLen(s);
            if (p < len) {
                if (isTile(s, label)) tile = s;
                break;
            }
            if (len > 0 && isTile(s, label)) tile = s;
            p -= len;
        }
    } else {
        let end = 0;
        for (const s of lv) end += localLen(s);
        if (pos > end) return -1;
        for (let i = lv.length - 1; i >= 0; i--) {
            const s = lv[i], len = localLen(s), at = end - len;
            if (pos >= at) {
                if (isTile(s, label)) tile = s;
                break;
            }
            if (len > 0 && isTile(s, label)) tile = s;
            end = at;
        }
    }
    return tile ? posOf(lv, tile) : -1;
}
function plainStack(lv, pos, label) {
    const st = [];
    const apply = (m) => {
        if (m.refType & NEST_BEGIN) st.push(m);
        else if (st.length && (st[st.length - 1].refType & NEST_BEGIN)) st.pop();
        else st.push(m);
    };
    let p = pos;
    for (const s of lv) {
        const len = localLen(s);
        if (p < len) {
            if (isRange(s, label)) apply(s);
            break;
        }
        if (len > 0 && isRange(s, label)) apply(s);
        p -= len;
    }
    return st.map((m) => [posOf(lv, m), m.refType]);
}

// ---- the farm
// cfg: ids (short ids of the clients, the logged one first), observer (the logged client edits nothing and
// is named "observer"), partial (the logged client lags), reconnect, offline, wide (content past the narrow
// limits), keys [tile key, range key], promoteAt (narrow until the logged client's own label annotate after
// that many edits: the label keys are wide), every (records between spread checkpoints)
function Farm(seed, cfg) {
    const r = rng(seed);
    const ri = (n) => Math.floor(r() * n);
    const ids = cfg.ids, own = cfg.observer ? 0 : ids[0], nClients = ids.length;
    const [tileKey, rangeKey] = cfg.keys;
    const clients = ids.map((id, i) => {
        const c = new Client(specToSegment, logger);
        c.startOrUpdateCollaboration(cfg.observer && i === 0 ? "observer" : "c" + id);
        return c;
    });
    const c1 = clients[0];
    const queue = [], seqd = [], cursor = clients.map(() => 0), log = [], cps = [];
    const counts = { local: 0, labelAnn: 0, labelLocal: 0, labelRewrite: 0, labelNull: 0, markers: 0, inserts: 0,
        pendingMax: 0, regenOps: 0 };
    let seq = 0, made = 0, labelPending = 0, promote = null, wide = !!cfg.wide, touched = [];
    const pendingNow = () => (c1.mergeTree.pendingSegments ? c1.mergeTree.pendingSegments.count() : 0);

    const kidOf = (k) => (k === TL ? tileKey : k === RL ? rangeKey : parseInt(k.slice(1), 10));
    const propsOut = (p) => {
        if (!p) return null;
        const o = {};
        for (const k of Object.keys(p)) {
            const v = p[k];
            o[kidOf(k)] = v === null || v === undefined ? null : Array.isArray(v) ? maskOf(v) : v;
        }
        return o;
    };
    const record = (s, ref, msn, client, op) => {
        if (op.type === 0) {
            const seg = op.seg;
            if (seg.marker) return [s, ref, msn, client, 0, op.pos1, 0, String.fromCharCode(seg.marker.refType), propsOut(seg.props), F_MARKER];
            const text = typeof seg === "string" ? seg : seg.text;
            return [s, ref, msn, client, 0, op.pos1, 0, text, typeof seg === "string" ? null : propsOut(seg.props), 0];
        }
        if (op.type === 1) return [s, ref, msn, client, 1, op.pos1, op.pos2, null, null, 0];
        return [s, ref, msn, client, 2, op.pos1, op.pos2, null, propsOut(op.props),
            op.combiningOp && op.combiningOp.name === "rewrite" ? F_REWRITE : 0];
    };
    const records = (s, ref, msn, client, op) => {
        if (op.type !== 3) return [record(s, ref, msn, client, op)];
        if (!op.ops.length) return [[s, ref, msn, client, 3, 0, 0, null, null, 0]];
        return op.ops.map((m, i) => {
            const x = record(s, ref, msn, client, m);
            if (i + 1 < op.ops.length) x[9] |= F_GROUP_MORE;
            return x;
        });
    };
    const isLabelAnn = (op) => (op.type === 3 ? op.ops.some(isLabelAnn) :
        op.type === 2 && (Object.prototype.hasOwnProperty.call(op.props, TL) || Object.prototype.hasOwnProperty.call(op.props, RL)));

    // the logged client's annotate and insert callbacks: the markers they touch are asked about next
    c1.mergeTreeDeltaCallback = (opArgs, args) => {
        if (args.operation !== 2 && args.operation !== 0) return;
        for (const d of args.deltaSegments) if (Marker.is(d.segment)) touched.push(d.segment);
    };

    const checkpoint = (why, extra) => {
        const k = log.length, len = c1.getLength();
        const lv = leavesOf(c1);
        const pos = [];
        const add = (p) => { if (p >= 0 && pos.length < MAX_POS && !pos.includes(p)) pos.push(p); };
        const last = cps.length && cps[cps.length - 1].k === k ? cps.pop() : null;
        if (last) { last.pos.forEach(add); why = last.why === "spread" ? why : last.why; }
        for (const p of [0, 1, 2, len >> 3, len >> 2, len >> 1, (3 * len) >> 2, len - 2, len - 1, len, len + 1]) add(p);
        for (const m of touched.concat(extra || [])) {
            if (m.parent === undefined) continue;
            const p = posOf(lv, m);
            add(p); add(p - 1); add(p + 1);
        }
        touched = [];
        pos.sort((a, b) => a - b);
        const tiles = [[], []], stacks = [[], []];
        let ptile = 0;
        for (const p of pos) {
            for (let l = 0; l < 4; l++) {
                for (const preceding of [true, false]) {
                    const t = c1.findTile(p, "L" + l, preceding);
                    tiles[0].push(t ? t.pos : -1);
                    if (t && t.tile.seq === -1) ptile++;
                    tiles[1].push(plainTile(lv, p, "L" + l, preceding));
                }
                const st = c1.getStackContext(p, ["L" + l])["L" + l];
                stacks[0].push(st ? st.items.map((m) => [c1.getPosition(m), m.refType]) : []);
                stacks[1].push(plainStack(lv, p, "L" + l));
            }
        }
        const removed = lv.filter((s) => Marker.is(s) && (s.refType & TILE) && s.removedSeq === -1).length;
        cps.push({ k, len, why, pend: [pendingNow(), labelPending], removed, pos, tiles, stacks, ptile });
    };
    let lastSpread = 0;
    // after every whole message / local edit of the logged client's log
    const logged = (recs, op) => {
        log.push(...recs);
        counts.pendingMax = Math.max(counts.pendingMax, pendingNow());
        if (op && isLabelAnn(op)) checkpoint("ann");
        else if (log.length - lastSpread >= cfg.every) checkpoint("spread");
        if (cps.length && cps[cps.length - 1].k === log.length) lastSpread = log.length;
    };
    const deliver = (i) => {
        const m = seqd[cursor[i]++];
        if (i !== 0) { clients[i].applyMsg(m); return; }
        const ack = !cfg.observer && m.clientId === "c" + own && isLabelAnn(m.contents);
        let ackMarkers;
        if (ack) {
            const sg = c1.mergeTree.pendingSegments.first();
            ackMarkers = sg.segments.filter((s) => Marker.is(s));
            checkpoint("pre", ackMarkers);
            labelPending--;
        }
        c1.applyMsg(m);
        log.push(...records(m.sequenceNumber, m.referenceSequenceNumber, m.minimumSequenceNumber,
            parseInt(m.clientId.slice(1), 10), m.contents));
        counts.pendingMax = Math.max(counts.pendingMax, pendingNow());
        if (ack) { checkpoint("ack", ackMarkers); lastSpread = log.length; } else logged([], m.contents);
    };
    // a local edit of client i: make(c) returns the op
    const local = (i, make) => {
        const c = clients[i];
        const op = make(c);
        if (!op) throw new Error("local op rejected");
        queue.push({ client: i, ref: c.getCurrentSeq(), op, sg: c.peekPendingSegmentGroups() });
        made++;
        if (i === 0) {
            counts.local++;
            if (isLabelAnn(op)) { labelPending++; counts.labelLocal++; }
            logged([record(-1, 0, 0, own, op)], op);
        }
        if (isLabelAnn(op)) {
            counts.labelAnn++;
            if (op.combiningOp) counts.labelRewrite++;
            if (op.props[TL] === null || op.props[RL] === null) counts.labelNull++;
        }
        return op;
    };
    const sequence = (holdOwn) => {
        const held = [];
        while (queue.length) {
            const q = queue.shift();
            if (holdOwn && q.client === 0) { held.push(q); continue; }
            seq++;
            const msn = Math.min(q.ref, ...clients.map((c) => c.getCurrentSeq()), ...queue.map((o) => o.ref),
                ...held.map((o) => o.ref));
            seqd.push({ clientId: "c" + ids[q.client], clientSequenceNumber: 1, contents: q.op, metadata: undefined,
                minimumSequenceNumber: msn, origin: undefined, referenceSequenceNumber: q.ref, sequenceNumber: seq,
                timestamp: 0, term: 1, traces: [], type: "op" });
        }
        queue.push(...held);
    };
    const deliverAll = (from) => { for (let i = from || 0; i < nClients; i++) while (cursor[i] < seqd.length) deliver(i); };

    // ---- drawn content
    const ch = (w) => {
        const p = w ? r() : 0;
        if (p < 0.5) return String.fromCharCode(97 + ri(26));
        if (p < 0.6) return String.fromCharCode(0xC0 + ri(0x3F));
        if (p < 0.85) return String.fromCharCode(0x4E00 + ri(0x5000));
        return String.fromCodePoint(0x1F600 + ri(64));
    };
    // a key that is no label key
    const keyOf = (w) => {
        for (;;) {
            const k = !w ? 2 + ri(2) : r() < 0.4 ? ri(8) : 8 + ri(24);
            if (k !== tileKey && k !== rangeKey) return k;
        }
    };
    const valOf = (w) => (!w ? 1 + ri(200) : r() < 0.6 ? 1 + ri(255) : r() < 0.9 ? 256 + ri(4000) : 65535 - ri(3));
    // a label array's mask: tiles any of 1..15; range markers one label, sometimes two (shallower stacks)
    const maskFor = (key) => (key === TL ? 1 + ri(15) : (1 << ri(4)) | (r() < 0.3 ? 1 << ri(4) : 0));
    const canLabel = () => wide || tileKey < 8;  // (a narrow document cannot carry wide label keys yet)
    const markersOf = (c) => {  // [[position, marker], ...] in the client's own view
        const out = [];
        let at = 0;
        for (const s of leavesOf(c)) {
            const len = localLen(s);
            if (len > 0 && Marker.is(s)) out.push([at, s]);
            at += len;
        }
        return out;
    };
    const labelAnnotate = (c, forceKey) => {
        const ms = markersOf(c);
        if (!ms.length) return undefined;
        const [p, m] = ms[ri(ms.length)];
        const len = c.getLength();
        const key = forceKey || ((m.refType & TILE) ? TL : RL);
        const props = {};
        props[key] = r() < 0.15 ? null : labelsOf(maskFor(key));
        const spread = r() < 0.25 ? 1 + ri(3) : 0;  // a range over the marker's neighbours too
        const a = Math.max(0, p - spread), b = Math.min(len, p + 1 + spread);
        return c.annotateRangeLocal(a, b, props, r() < 0.12 ? { name: "rewrite" } : undefined);
    };
    const localOp = (i) => {
        const c = clients[i];
        const len = c.getLength();
        const w = wide;
        const pick = r();
        return local(i, () => {
            if (len === 0 || pick < 0.42) {
                counts.inserts++;
                let seg, props;
                if (r() < 0.34) {
                    counts.markers++;
                    const rt = [TILE, TILE, NEST_BEGIN, NEST_END][ri(4)];
                    seg = new Marker(rt);
                    if (canLabel() && r() < 0.9) { props = {}; props[rt === TILE ? TL : RL] = labelsOf(maskFor(rt === TILE ? TL : RL)); }
                    if (w && r() < 0.3) { props = props || {}; props["k" + keyOf(w)] = valOf(w); }
                } else {
                    const n = 1 + ri(4);
                    let text = "";
                    for (let q = 0; q < n; q++) text += ch(w);
                    seg = new TextSegment(text);
                    if (r() < 0.25) { props = {}; props["k" + keyOf(w)] = valOf(w); }
                }
                if (props) seg.addProperties(props);
                return c.insertSegmentLocal(ri(len + 1), seg);
            }
            if (pick < 0.6) {
                const a = ri(len), b = a + 1 + ri(Math.min(6, len - a));
                return c.removeRangeLocal(a, b);
            }
            if (pick < 0.64 && canLabel()) {
                const op = labelAnnotate(c);
                if (op) return op;
            }
            const a = ri(len), b = a + 1 + ri(Math.min(14, len - a));
            const props = {};
            const nk = 1 + ri(w ? 3 : 2);
            for (let q = 0; q < nk; q++) props["k" + keyOf(w)] = r() < 0.15 ? null : valOf(w);
            return c.annotateRangeLocal(a, b, props, r() < 0.1 ? { name: "rewrite" } : undefined);
        });
    };

    // ---- the drawn run (the rounds of localw_ref.js)
    const run = (nOps) => {
        let away = 0;
        while (made < nOps) {
            if (cfg.offline && !away && r() < 0.08) away = 14 + ri(12);
            if (cfg.promoteAt !== undefined && !wide && made >= cfg.promoteAt) {
                // the promoting round: a marker of the logged client's own, then its label annotate -- a
                // wide record -- with edits pending
                local(0, (c) => c.insertSegmentLocal(ri(c.getLength() + 1), new Marker(TILE)));
                wide = true;
                const at = log.length;
                local(0, (c) => labelAnnotate(c, TL));
                promote = { k: at, pending: pendingNow() };
            }
            for (let i = cfg.observer ? 1 : 0; i < nClients; i++) {
                const k = away && i === 0 ? 2 + ri(5) : r() < 0.6 ? 1 + ri(3) : 0;
                for (let q = 0; q < k; q++) localOp(i);
            }
            let lost = [];
            if (cfg.reconnect && r() < 0.5) {
                lost = queue.filter((q) => q.client === 0);
                for (let q = queue.length - 1; q >= 0; q--) if (queue[q].client === 0) queue.splice(q, 1);
            }
            sequence(away > 0);
            deliverAll(1);
            if (away) { away--; continue; }
            const upto = cfg.partial ? cursor[0] + ri(seqd.length - cursor[0] + 1) : seqd.length;
            while (cursor[0] < upto) deliver(0);
            for (const q of lost) {
                const recs = records(-2, 0, 0, own, q.op);
                const op = c1.regeneratePendingOp(q.op, q.sg);
                counts.regenOps += op.type === 3 ? op.ops.length : 1;
                // (the regenerated op takes the lost one's place: a lost label annotate stays pending)
                queue.push({ client: 0, ref: c1.getCurrentSeq(), op, sg: undefined });
                if (isLabelAnn(q.op) && !isLabelAnn(op)) labelPending--;
                logged(recs, q.op);  // (a reset label annotate is asked about too)
            }
            if (lost.length) {
                sequence(false);
                deliverAll(0);
            }
        }
    };
    const finish = () => {
        sequence(false);
        deliverAll(0);
        const text = (c) => c.createTextHelper().getText(c.getCurrentSeq(), c.getClientId());
        const t0 = text(c1);
        for (const c of clients) if (text(c) !== t0) return null;  // the reference's clients diverged: dropped
        if (pendingNow() !== 0) return null;
        checkpoint("end");
        // queries whose answer differs between the two checkpoints around the ack of a local label annotate
        let ackFlips = 0;
        for (let q = 1; q < cps.length; q++) {
            const a = cps[q - 1], b = cps[q];
            if (b.why !== "ack") continue;
            if (a.len !== b.len) throw new Error("an ack changed the local view");
            a.pos.forEach((p, ia) => {
                const ib = b.pos.indexOf(p);
                if (ib < 0) return;
                for (let j = 0; j < 8; j++) if (a.tiles[0][8 * ia + j] !== b.tiles[0][8 * ib + j]) ackFlips++;
                for (let j = 0; j < 4; j++) {
                    if (JSON.stringify(a.stacks[0][4 * ia + j]) !== JSON.stringify(b.stacks[0][4 * ib + j])) ackFlips++;
                }
            });
        }
        counts.ackFlips = ackFlips;
        return { ids, observer: !!cfg.observer, keys: cfg.keys, records: log, checkpoints: cps, counts, promote,
            segs: leavesOf(c1).length };
    };
    return { r, ri, clients, c1, local, localOp, sequence, deliver, deliverAll, checkpoint, run, finish, cursor, seqd,
        queue, log, pendingNow };
}

// ---- tf_scenarios: hand-written, deterministic
function scenario(which) {
    const editing = which !== "f";
    const F = Farm(1, { ids: editing ? [1, 2, 3] : [0, 1, 2, 3], observer: !editing, keys: [0, 1], every: 8 });
    const tile = (mask) => { const m = new Marker(TILE); m.addProperties({ [TL]: labelsOf(mask) }); return m; };
    const nest = (rt, mask) => { const m = new Marker(rt); m.addProperties({ [RL]: labelsOf(mask) }); return m; };
    const all = () => { F.sequence(false); F.deliverAll(0); };
    const remote = (i, make) => { F.local(i, make); };
    // the ack (or remote message) alone: sequenced, delivered to everyone, the logged client last
    const flushOthersFirst = () => { F.sequence(false); F.deliverAll(1); F.deliverAll(0); };
    if (which !== "e") {
        // ten tiles L0 with text between them: three leaf blocks (tiles_annot's first shape)
        for (let k = 0; k < 10; k++) {
            remote(1, (c) => c.insertSegmentLocal(2 * k, tile(1)));
            all();
            remote(1, (c) => c.insertSegmentLocal(2 * k + 1, new TextSegment("x")));
            all();
        }
    } else {
        // begins and ends, nested: every third an end; labels R0 on begins, R1 on ends
        for (let k = 0; k < 12; k++) {
            remote(1, (c) => c.insertSegmentLocal(2 * k, k % 3 ? nest(NEST_BEGIN, 1) : nest(NEST_END, 2)));
            all();
            remote(1, (c) => c.insertSegmentLocal(2 * k + 1, new TextSegment("y")));
            all();
        }
    }
    F.checkpoint("spread");
    if (which === "a") {
        F.local(0, (c) => c.annotateRangeLocal(8, 9, { [TL]: labelsOf(2) }));
        flushOthersFirst();
        // again on another block's tile, to null, then a rewrite
        F.local(0, (c) => c.annotateRangeLocal(16, 17, { [TL]: null }));
        flushOthersFirst();
        F.local(0, (c) => c.annotateRangeLocal(2, 3, { [TL]: labelsOf(4) }, { name: "rewrite" }));
        flushOthersFirst();
    } else if (which === "b") {
        F.local(0, (c) => c.annotateRangeLocal(8, 9, { [TL]: labelsOf(2) }));
        remote(1, (c) => c.annotateRangeLocal(8, 9, { [TL]: labelsOf(4) }));
        // the remote annotate is sequenced first and arrives while the local one is pending
        const mine = F.queue.splice(0, 1);
        F.sequence(false);
        F.deliverAll(0);
        F.queue.push(...mine);
        flushOthersFirst();
        F.local(0, (c) => c.annotateRangeLocal(12, 13, { [TL]: labelsOf(8) }));
        remote(2, (c) => c.annotateRangeLocal(12, 13, { [TL]: null }));
        flushOthersFirst();  // (here the local one is sequenced first)
    } else if (which === "c") {
        F.local(0, (c) => c.insertSegmentLocal(9, tile(4)));
        F.checkpoint("spread");
        flushOthersFirst();
        F.checkpoint("spread");
        F.local(0, (c) => c.insertSegmentLocal(0, tile(1)));
        F.local(0, (c) => c.insertSegmentLocal(c.getLength(), tile(2)));
        F.checkpoint("spread");
        flushOthersFirst();
        F.checkpoint("spread");
    } else if (which === "d") {
        F.local(0, (c) => c.removeRangeLocal(8, 9));
        F.checkpoint("spread");
        remote(1, (c) => c.removeRangeLocal(8, 9));  // (made without the local removal: the same tile)
        const mine = F.queue.splice(0, 1);
        F.sequence(false);
        F.deliverAll(0);
        F.checkpoint("spread");
        F.queue.push(...mine);
        flushOthersFirst();
        F.checkpoint("spread");
        F.local(0, (c) => c.removeRangeLocal(0, 1));
        F.checkpoint("spread");
        flushOthersFirst();
        F.checkpoint("spread");
    } else if (which === "e") {
        F.local(0, (c) => c.annotateRangeLocal(2, 3, { [RL]: labelsOf(2) }));   // a begin R0 -> R1
        flushOthersFirst();
        F.local(0, (c) => c.annotateRangeLocal(6, 7, { [RL]: labelsOf(1) }));   // an end R1 -> R0
        flushOthersFirst();
        F.local(0, (c) => c.insertSegmentLocal(9, nest(NEST_BEGIN, 3)));
        F.checkpoint("spread");
        F.local(0, (c) => c.insertSegmentLocal(15, nest(NEST_END, 1)));
        F.checkpoint("spread");
        flushOthersFirst();
        F.checkpoint("spread");
        F.local(0, (c) => c.annotateRangeLocal(14, 15, { [RL]: null }));
        flushOthersFirst();
    } else {
        for (const a of [4, 8, 12]) {
            remote(2, (c) => c.annotateRangeLocal(a, a + 1, { [TL]: labelsOf(2) }));
            all();
        }
        remote(3, (c) => c.insertSegmentLocal(1, new TextSegment("ins")));
        all();
    }
    // a tail of edits after the case, so the stale blocks get refreshed one by one
    remote(1, (c) => c.insertSegmentLocal(1, new TextSegment("t")));
    all();
    F.checkpoint("spread");
    remote(2, (c) => c.removeRangeLocal(c.getLength() - 2, c.getLength() - 1));
    all();
    F.checkpoint("spread");
    return F.finish();
}

const KINDS = {
    edit: { ids: [1, 2, 3, 4], keys: [0, 1] },
    edit_lag: { ids: [1, 2, 3, 4], keys: [0, 1], partial: true },
    edit_reconnect: { ids: [1, 2, 3, 4], keys: [0, 1], reconnect: true },
    edit_offline: { ids: [1, 2, 3, 4], keys: [0, 1], offline: true },
    wide: { ids: [0, 1, 2, 70, 300], keys: [20, 27], observer: true, wide: true, partial: true },
    edit_wide: { ids: [1, 2, 70, 300], keys: [20, 27], wide: true, partial: true },
};

function main() {
    const [kind, seedS, nDocsS, nOpsS] = process.argv.slice(2);
    const seed = parseInt(seedS, 10), nDocs = parseInt(nDocsS, 10), nOps = parseInt(nOpsS, 10);
    let tried = 0, dropped = 0;
    const out = [];
    if (kind === "scenarios") {
        for (const which of ["a", "b", "c", "d", "e", "f"]) {
            tried++;
            const doc = scenario(which);
            if (!doc) throw new Error("scenario " + which + " diverged");
            doc.name = "scenario_" + which;
            out.push(doc);
        }
    }
    for (let d = 0; kind !== "scenarios" && d < nDocs;) {
        const cfg = Object.assign({ every: 30 }, KINDS[kind]);
        // tf_edit_wide: its last two documents start narrow and turn wide with a label annotate pending
        const promoting = kind === "edit_wide" && d >= nDocs - 2;
        if (promoting) { cfg.wide = false; cfg.promoteAt = 30; cfg.ids = [1, 2, 3, 4]; }
        const s = seed * 7919 + tried;
        tried++;
        let doc = null;
        try {
            const F = Farm(s, cfg);
            F.run(nOps);
            doc = F.finish();
        } catch (e) {
            if (process.env.TILEFORMS_DEBUG) console.error(e.stack);
            doc = null;
        }
        const ok = doc && doc.checkpoints.length >= 8 && (!promoting || (doc.promote && doc.promote.pending > 1)) &&
            (kind !== "edit_offline" || doc.counts.pendingMax > 64);
        if (!ok) { dropped++; continue; }
        doc.name = `${kind}_${d}`;
        out.push(doc);
        d++;
    }
    for (const doc of out) process.stdout.write(JSON.stringify(doc) + "\n");
    process.stdout.write(JSON.stringify({ tried, kept: out.length, dropped }) + "\n");
}
main();
