"use strict";
// Marker-relative ops on the REFERENCE (the transpile under oracle/_tsref): a farm of reference Clients
// in the lagging pattern of oracle/tsref/local_farm.js whose clients insert text and markers with ids,
// remove ranges and annotate markers through Client.annotateMarker (client.ts:142-154), which sends an
// ANNOTATE with relativePos1 {id, before: true} / relativePos2 {id} (opBuilder.ts:25-39) that every
// receiver resolves against its own tree (client.ts:485-502, mergeTree.ts:1943-1966).
//
//   node relpos_ref.js <cfg.json> -> one JSON line per document:
//     {observer: {records, checkpoints, rel, events, pfr}, c1: {...the same...} | null, messages, counts}
//   cfg: {docs, seed, ops, clients: [client numbers, the first is the editing client c<n> whose view
//         is logged], markerKey, firstId, unknownId, wide, views: ["observer", "c1"], every, phantom, extra: [...]}
// Marker ids are "m<n>" from a counter (n from firstId up, unique in the document); in the records the
// id travels as value id n of property key `markerKey`, and a relative end as {key, value, before,
// offset}.  extra: hand-written ops sent by client c<phantom> at given rounds (make_relpos.py): an unknown
// id, offsets on both sides, a relative REMOVE, a relative INSERT, a GROUP with a relative member.
//
//   records      [seq, ref, msn, client, type, pos1, pos2, text | null, {key id: value id | null} | null,
//                 flags, rel1 | null, rel2 | null]   (c1's local edits: seq -1, as local_farm.js writes)
//   checkpoints  [{k, state}]: the canonical state (DESIGN.md "Canonical state") after k records
//   rel          [[record index, start, end, kind, splits]] per relative record the client RESOLVED
//                (not its own acks): getValidOpRange's range; kind "live" | "tomb" (the marker is removed
//                at this client) | "none" (no such id: -1, -1); splits: SPLIT callbacks it caused;
//                on c1 two more fields: pending segments before / after the marker
//   events       the client's callbacks, in replay_ref.js' canonical form [seq, operation, [[leaf, pos,
//                len, propertyDeltas]]]
//   pfr          [[k, view | null, value id, before, offset | null, answer]] posFromRelativePos at
//                checkpoints: view null = Client.posFromRelativePos (the local view), [refSeq, client] =
//                MergeTree.posFromRelativePos(rel, refSeq, clientId) for that client's latest op's pair
//   messages     the sequenced ISequencedDocumentMessage stream (JSON), for the Node shim's replay
// A sender draws its target among the markers that are live in its local view or under its own pending
// removal, so the marker is linked at every receiver (msn <= refSeq < its removal's seq): `skipped`
// counts relative ops whose marker a receiver had already unlinked, and must stay 0.
const fs = require("fs");
const path = require("path");

const ROOT = path.join(__dirname, "..", "..", "oracle", "_tsref", "merge-tree", "src");
const { Client } = require(path.join(ROOT, "client.js"));
const { TextSegment } = require(path.join(ROOT, "textSegment.js"));
const { Marker } = require(path.join(ROOT, "mergeTree.js"));

function specToSegment(spec) { return TextSegment.fromJSONObject(spec) || Marker.fromJSONObject(spec); }
const logger = { send() {}, sendTelemetryEvent() {}, sendErrorEvent() {}, sendPerformanceEvent() {} };

function rng(seed) {  // xorshift32
    let s = seed >>> 0 || 1;
    return () => {
        s ^= s << 13; s >>>= 0; s ^= s >>> 17; s ^= s << 5; s >>>= 0;
        return s / 4294967296;
    };
}

const F_REWRITE = 1, F_GROUP_MORE = 4, F_MARKER = 128;
const idValue = (id) => parseInt(id.slice(1), 10);

function run(cfg, seed) {
    const MK = cfg.markerKey;
    const r = rng(seed);
    const ri = (n) => Math.floor(r() * n);
    const numOf = (long) => (long === "observer" ? 0 : parseInt(long.slice(1), 10));
    const logId = (c, shortId) => (shortId < 0 ? -2 : numOf(c.getLongClientId(shortId)));
    const propsOut = (p) => {  // {key id: value id | null}, the marker id under markerKey
        if (!p) return null;
        const o = {};
        for (const k of Object.keys(p)) {
            const v = p[k] === undefined ? null : p[k];
            if (k === "markerId") o[MK] = v === null ? null : idValue(v); else o[parseInt(k.slice(1), 10)] = v;
        }
        return o;
    };
    const relOut = (rp) => (rp ? { key: MK, value: rp.id === undefined ? 0 : idValue(rp.id), before: !!rp.before,
        offset: rp.offset === undefined ? 0 : rp.offset } : null);
    function record(seq, ref, msn, client, op) {
        const r1 = op.pos1 === undefined ? relOut(op.relativePos1) : null;
        const r2 = op.pos2 === undefined ? relOut(op.relativePos2) : null;
        const p1 = op.pos1 === undefined ? 0 : op.pos1, p2 = op.pos2 === undefined ? 0 : op.pos2;
        if (op.type === 0) {
            const seg = op.seg;
            if (seg.marker) {
                return [seq, ref, msn, client, 0, p1, 0, String.fromCharCode(seg.marker.refType), propsOut(seg.props),
                    F_MARKER, r1, null];
            }
            const text = typeof seg === "string" ? seg : seg.text;
            return [seq, ref, msn, client, 0, p1, 0, text, typeof seg === "string" ? null : propsOut(seg.props), 0, r1, null];
        }
        if (op.type === 1) return [seq, ref, msn, client, 1, p1, p2, null, null, 0, r1, r2];
        return [seq, ref, msn, client, 2, p1, p2, null, propsOut(op.props),
            op.combiningOp && op.combiningOp.name === "rewrite" ? F_REWRITE : 0, r1, r2];
    }
    function records(seq, ref, msn, client, op) {
        if (op.type !== 3) return [record(seq, ref, msn, client, op)];
        return op.ops.map((m, i) => {
            const x = record(seq, ref, msn, client, m);
            if (i + 1 < op.ops.length) x[9] |= F_GROUP_MORE;
            return x;
        });
    }
    const leaves = (c) => {
        const out = [];
        const walk = (b) => {
            for (let i = 0; i < b.childCount; i++) {
                const ch = b.children[i];
                if (!ch.isLeaf()) walk(ch); else out.push(ch);
            }
        };
        walk(c.mergeTree.root);
        return out;
    };
    function canonical(c) {
        const segs = leaves(c).map((ch) => {
            const removed = ch.removedSeq !== undefined;
            const ov = (ch.removedClientOverlap || []).map((x) => logId(c, x)).sort((a, b) => a - b);
            let props = null;
            if (ch.properties) {
                const o = propsOut(ch.properties);
                props = {};
                for (const k of Object.keys(o).map((x) => parseInt(x, 10)).sort((a, b) => a - b)) props["k" + k] = o[k];
            }
            return [Marker.is(ch) ? { marker: ch.refType } : ch.text, ch.seq, logId(c, ch.clientId), removed ? ch.removedSeq : -1,
                removed ? logId(c, ch.removedClientId) : -1, ov, props];
        });
        const tree = [];
        let lvl = [c.mergeTree.root];
        while (lvl.length) {
            tree.push(lvl.map((b) => b.childCount));
            const nxt = [];
            for (const b of lvl) for (let i = 0; i < b.childCount; i++) if (!b.children[i].isLeaf()) nxt.push(b.children[i]);
            lvl = nxt;
        }
        const w = c.mergeTree.getCollabWindow();
        return { seq: w.currentSeq, msn: w.minSeq, segs, tree };
    }
    // a logged client: its records, and what the reference did with them
    function view(c) {
        const v = { c, records: [], checkpoints: [], rel: [], events: [], pfr: [], seq: 0, splits: 0, seen: new Map(),
            lastCk: 0 };
        const where = (seg) => {
            let ord = 0, pos = 0;
            for (const ch of leaves(c)) {
                if (ch.parent === undefined) continue;
                if (ch === seg) return [ord, pos];
                ord++;
                pos += ch.removedSeq === undefined ? ch.cachedLength : 0;
            }
            return [-1, -1];
        };
        const pdelta = (pd) => {
            if (!pd) return null;
            const o = propsOut(pd), out = {};
            for (const k of Object.keys(o).map((x) => parseInt(x, 10)).sort((a, b) => a - b)) out["k" + k] = o[k];
            return out;
        };
        c.mergeTreeDeltaCallback = (opArgs, args) => {
            v.events.push([v.seq, args.operation, args.deltaSegments.map((d) => {
                const [leaf, pos] = where(d.segment);
                return [leaf, pos, d.segment.cachedLength, args.operation === 2 ? pdelta(d.propertyDeltas) : null];
            })]);
        };
        c.mergeTreeMaintenanceCallback = (args) => {
            const segs = [];
            for (let i = 0; i < args.deltaSegments.length; i++) {
                const seg = args.deltaSegments[i].segment;
                let leaf = where(seg)[0];
                if (args.operation === -2 && i === 1) leaf = segs[0][0] + 1;
                segs.push([leaf, -1, seg.cachedLength, null]);
            }
            if (args.operation === -2) v.splits++;
            v.events.push([v.seq, args.operation, segs]);
        };
        // what getValidOpRange (client.ts:485-547) answers, for remote members and for the client's own edits
        const orig = c.getValidOpRange.bind(c);
        c.getValidOpRange = (op, args) => {
            const range = orig(op, args);
            v.lastRange = range ? [range.start, range.end] : null;
            if (v.hook) v.hook(op, range);
            return range;
        };
        return v;
    }
    const counts = { rel: 0, live: 0, tomb: 0, split: 0, none: 0, ord64: 0, ord128: 0, pend_before: 0, pend_after: 0,
        skipped: 0, pfr: 0, pfr_remote: 0, pfr_differs: 0, insert_rel: 0, remove_rel: 0, group_rel: 0, offsets: 0 };
    const ids = [];          // every id handed out
    let nextId = cfg.firstId;
    // one relative member as the client resolved it: `range` is what its getValidOpRange returned, and the
    // tree is still in the state the member was resolved in
    function noteRel(v, m, range, index) {
        const c = v.c, mt = c.mergeTree;
        const rp = m.pos1 === undefined ? m.relativePos1 : m.relativePos2;
        const marker = rp.id !== undefined ? mt.getMarkerFromId(rp.id) : undefined;
        let kind = "none";
        const row = [index, range.start, range.end === undefined ? 0 : range.end, kind, 0];
        if (marker) {
            if (marker.parent === undefined) { counts.skipped++; return null; }
            kind = marker.removedSeq !== undefined ? "tomb" : "live";
            const all = leaves(c);
            const ord = all.indexOf(marker);
            if (ord >= 64) counts.ord64++;
            if (ord >= 128) counts.ord128++;
            if (v.own) {
                const pend = (x) => x.seq === -1 || x.removedSeq === -1;
                const pb = all.slice(0, ord).filter(pend).length, pa = all.slice(ord + 1).filter(pend).length;
                if (pb) counts.pend_before++;
                if (pa) counts.pend_after++;
                row.push(pb, pa);
            }
        } else if (v.own) row.push(0, 0);
        row[3] = kind;
        counts.rel++;
        counts[kind]++;
        if (m.type === 0) counts.insert_rel++;
        if (m.type === 1) counts.remove_rel++;
        if ((m.relativePos1 && m.relativePos1.offset) || (m.relativePos2 && m.relativePos2.offset)) counts.offsets++;
        return row;
    }
    const isRel = (m) => m.pos1 === undefined || (m.type !== 0 && m.pos2 === undefined);
    function apply(v, msg) {
        const c = v.c;
        const mine = v.own && msg.clientId === c.longClientId;
        const base = v.records.length;
        v.records.push(...records(msg.sequenceNumber, msg.referenceSequenceNumber, msg.minimumSequenceNumber,
            numOf(msg.clientId), msg.contents));
        v.seq = msg.sequenceNumber;
        // every member of the message passes through getValidOpRange once, in order (an ack does not)
        let member = 0, open = null, s0 = 0;
        const close = () => {
            if (open) {
                open[4] = v.splits - s0;
                if (open[4]) counts.split++;
                v.rel.push(open);
            }
            open = null;
        };
        v.hook = (op, range) => {
            close();
            if (isRel(op) && range) {
                open = noteRel(v, op, range, base + member);
                s0 = v.splits;
                if (msg.contents.type === 3) counts.group_rel++;
            }
            member++;
        };
        c.applyMsg(msg);
        close();
        v.hook = null;
        if (!mine) v.seen.set(numOf(msg.clientId), [msg.referenceSequenceNumber, numOf(msg.clientId)]);
    }
    function checkpoint(v) {
        const c = v.c, k = v.records.length;
        if (v.checkpoints.length && v.checkpoints[v.checkpoints.length - 1].k === k) return;
        v.checkpoints.push({ k, state: canonical(c) });
        v.lastCk = k;
        if (!ids.length) return;
        const minSeq = c.getCollabWindow().minSeq;
        const views = [null];
        if (!v.own) for (const x of [...v.seen.values()].filter((y) => y[0] >= minSeq).sort((a, b) => a[1] - b[1])) views.push(x);
        for (let q = 0; q < 6; q++) {
            const id = r() < 0.1 ? "m" + cfg.unknownId : ids[ri(ids.length)];
            const before = r() < 0.5;
            const offset = r() < 0.3 ? ri(5) - 1 : undefined;
            const vw = views[ri(views.length)];
            const rp = { id, before };
            if (offset !== undefined) rp.offset = offset;
            let ans;
            const marker = c.mergeTree.getMarkerFromId(id);
            if (marker && marker.parent === undefined) continue;  // (unlinked by zamboni: a kept difference)
            if (vw === null) ans = c.posFromRelativePos(rp);
            else ans = c.mergeTree.posFromRelativePos(rp, vw[0], c.getOrAddShortClientId("c" + vw[1]));
            counts.pfr++;
            if (vw !== null) {
                counts.pfr_remote++;
                if (ans !== c.posFromRelativePos(rp)) counts.pfr_differs++;
            }
            v.pfr.push([k, vw, idValue(id), before, offset === undefined ? null : offset, ans]);
        }
    }

    const clients = cfg.clients.map((n) => {
        const c = new Client(specToSegment, logger);
        c.startOrUpdateCollaboration("c" + n);
        return c;
    });
    const observer = new Client(specToSegment, logger);
    observer.startOrUpdateCollaboration("observer");
    const ov = view(observer);
    const c1v = cfg.views.includes("c1") ? view(clients[0]) : null;
    if (c1v) { c1v.own = true; c1v.seq = -1; }
    const nClients = clients.length;
    const queue = [], seqd = [], cursor = clients.map(() => 0);
    let seq = 0, made = 0, round = 0;
    const deliver = (i) => {
        const m = seqd[cursor[i]++];
        if (i === 0 && c1v) {
            apply(c1v, m);
            c1v.seq = -1;
            if (c1v.records.length - c1v.lastCk >= cfg.every) checkpoint(c1v);
        } else clients[i].applyMsg(m);
    };
    const ch = () => String.fromCharCode(cfg.wide && r() < 0.3 ? 0x3b1 + ri(24) : 97 + ri(26));
    const submit = (i, op) => {
        const c = clients[i];
        queue.push({ client: cfg.clients[i], ref: c.getCurrentSeq(), op });
        made++;
    };
    const localOp = (i) => {
        const c = clients[i];
        const len = c.getLength();
        const pick = r();
        let op;
        const mine = leaves(c).filter((x) => x.parent !== undefined && Marker.is(x) && x.getId() !== undefined &&
            (x.removedSeq === undefined || x.removedSeq === -1));
        if (mine.length && pick < 0.22) {
            const props = {};
            props["k" + ri(3)] = r() < 0.15 ? null : 1 + ri(4);
            // (a rewrite drops every key it does not name: it names the id again, or the marker would lose it
            // -- the reference's id map would still hold it, a kept difference the fixture stays clear of)
            const target = mine[ri(mine.length)];
            const rewrite = r() < 0.1;
            if (rewrite) props.markerId = target.getId();
            op = c.annotateMarker(target, props, rewrite ? { name: "rewrite" } : undefined);
            if (!op) return;  // (a pending-removed marker at the end of the local view: no valid range)
            if (i === 0 && c1v) c1v.records.push(record(-1, 0, 0, cfg.clients[0],
                { type: 2, pos1: c1v.lastRange[0], pos2: c1v.lastRange[1], props: op.props, combiningOp: op.combiningOp }));
            submit(i, op);
            return;
        }
        if (len === 0 || pick < 0.66) {
            const n = 1 + ri(4);
            let text = "";
            for (let q = 0; q < n; q++) text += ch();
            let props;
            if (r() < 0.25) { props = {}; props["k" + ri(3)] = 1 + ri(4); }
            let seg;
            if (r() < 0.3) {
                seg = new Marker([0, 1, 2, 4][ri(4)]);
                const id = "m" + nextId++;
                ids.push(id);
                props = Object.assign(props || {}, { markerId: id });
            } else seg = new TextSegment(text);
            if (props) seg.addProperties(props);
            op = c.insertSegmentLocal(ri(len + 1), seg);
        } else {
            const a = ri(len), b = a + 1 + ri(Math.min(4, len - a));
            if (pick < 0.82) op = c.removeRangeLocal(a, b);
            else {
                const props = {};
                props["k" + ri(3)] = r() < 0.15 ? null : 1 + ri(4);
                op = c.annotateRangeLocal(a, b, props, undefined);
            }
        }
        if (!op) throw new Error("local op rejected");
        if (i === 0 && c1v) c1v.records.push(record(-1, 0, 0, cfg.clients[0], op));
        submit(i, op);
    };
    const sequenceAll = () => {
        while (queue.length) {
            const q = queue.shift();
            seq++;
            const msn = Math.min(q.ref, ...clients.map((c) => c.getCurrentSeq()), ...queue.map((o) => o.ref));
            const m = { clientId: "c" + q.client, clientSequenceNumber: 1, contents: q.op, metadata: undefined,
                minimumSequenceNumber: msn, origin: undefined, referenceSequenceNumber: q.ref, sequenceNumber: seq,
                timestamp: 0, term: 1, traces: [], type: "op" };
            seqd.push(m);
            apply(ov, m);
            if (ov.records.length - ov.lastCk >= cfg.every) checkpoint(ov);
        }
    };
    const extra = (cfg.extra || []).slice();
    while (made < cfg.ops || extra.length) {
        round++;
        for (let i = 0; i < nClients; i++) {
            const k = r() < 0.6 ? 1 + ri(3) : 0;
            for (let q = 0; q < k; q++) localOp(i);
        }
        // hand-written ops, from a sender that is no reference Client (cfg.phantom: it keeps no tree, and is
        // up to date with everything sequenced when it sends): the forms annotateMarker never produces
        while (extra.length && extra[0].round <= round) {
            const x = extra.shift();
            const fill = (m) => {
                const o = JSON.parse(JSON.stringify(m));
                for (const key of ["relativePos1", "relativePos2"]) {
                    if (o[key] && o[key].id === "$any") {
                        // a marker live at the observer (the sender's view: it has seen everything sequenced), at
                        // least x.minPos units into the text
                        const live = leaves(observer).filter((y) => Marker.is(y) && y.getId() !== undefined && y.removedSeq === undefined &&
                            observer.getPosition(y) >= (x.minPos || 0));
                        if (!live.length) return null;
                        o[key].id = live[(x.pick || 0) % live.length].getId();
                    }
                }
                if (o.props && o.props.markerId === "$id") o.props.markerId = o.relativePos1.id;
                if (o.type === 0 && o.seg && o.seg.marker && o.seg.props && o.seg.props.markerId === "$new") {
                    o.seg.props.markerId = "m" + nextId++;
                    ids.push(o.seg.props.markerId);
                }
                return o;
            };
            const op = x.op.type === 3 ? { type: 3, ops: x.op.ops.map(fill) } : fill(x.op);
            if (!op || (op.ops && op.ops.some((m) => !m))) { x.round = round + 1; extra.unshift(x); break; }
            queue.push({ client: cfg.phantom, ref: seq, op });
        }
        sequenceAll();
        for (let i = 1; i < nClients; i++) while (cursor[i] < seqd.length) deliver(i);
        const upto = cursor[0] + ri(seqd.length - cursor[0] + 1);
        while (cursor[0] < upto) deliver(0);
    }
    while (cursor[0] < seqd.length) deliver(0);
    checkpoint(ov);
    if (c1v) checkpoint(c1v);
    const txt = (c) => c.createTextHelper().getText(c.getCurrentSeq(), c.getClientId());
    const t0 = txt(observer);
    for (const c of clients) if (txt(c) !== t0) return null;  // the reference's clients diverged: drop the run
    const out = (v) => ({ records: v.records, checkpoints: v.checkpoints, rel: v.rel, events: v.events, pfr: v.pfr });
    return { observer: out(ov), c1: c1v ? out(c1v) : null, messages: seqd, counts };
}

const cfg = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));
let dropped = 0;
const lines = [];
for (let d = 0, k = 0; d < cfg.docs; k++) {
    const res = run(cfg, cfg.seed * 7919 + k);
    if (res) { lines.push(JSON.stringify(res)); d++; } else dropped++;
    if (dropped > 200) throw new Error("relpos_ref: too many diverged runs");
}
process.stderr.write(`relpos_ref: ${cfg.docs} documents, ${dropped} runs dropped (clients diverged)\n`);
process.stdout.write(lines.join("\n") + "\n");
