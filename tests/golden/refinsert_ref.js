"use strict";
// Client.insertAtReferencePositionLocal on the REFERENCE merge-tree (the transpile under oracle/_tsref):
// hand-written scenarios and a farm, both seen from the editing client "c1", for make_refinsert.py.
//
//   node refinsert_ref.js scenarios            -> JSON lines, one per scenario document
//   node refinsert_ref.js farm <seed> <runs> <ops> <lag 0|1>   -> JSON lines, one per kept run, then
//                                                 one line {dropped, tried}
// A document line: {name, records, refs, ats, checkpoints, counts[, marker]}
//   records      c1's log (oracle/tsref/local_farm.js's tuples): [seq, ref, msn, client, type, pos1, pos2, text,
//                props {key id: value id | null} | null, flags]; c1's local edits have seq -1; an
//                insertAtReferencePositionLocal is a local record of type 5 (MT_OP_INSERT_AT) whose pos1
//                is the fixture's reference id (a host lowers it through mt_refs_insert_local)
//   refs         [[k, id, pos, refType], ...]: before record k, new LocalReference at
//                getContainingSegment(pos) of the local view + addLocalReference; ids count from 0
//   ats          one per type-5 record, in order: {k, id, op: returned pos1 | null} and, when applied,
//                {ord, n, levels, split, refOrd, refOff, pre, left, moved, zero, first, differs, refs, ev[, state]}:
//                the new leaf's ordinal, the leaf count, the blocks per level (root first), whether the
//                reference's leaf was split, the reference's leaf ordinal and getOffset() before the call,
//                one character per leaf before the call ('.' live, 'x' removed and acked, 'p' removal
//                pending), whether the new leaf landed left of the reference's segment (not inside it), whether it
//                passed leaves without local length on the way (the left excursion), whether the reference's
//                leaf had no local length, whether the new leaf is the first child of a leaf block other
//                than the first, whether the leaves differ from insertSegmentLocal(op.pos1) on a replay of
//                the same log, every reference's [toPosition(), ordinal, getOffset()] afterwards (0: detached),
//                the callbacks fired inside the call (oracle/tsref/replay_ref.js's form)
//   checkpoints  [{k, state}]: canonical states (replay_ref.js) after k records; the last is the end
const path = require("path");

const ROOT = path.join(__dirname, "..", "..", "oracle", "_tsref", "merge-tree", "src");
const { Client } = require(path.join(ROOT, "client.js"));
const { TextSegment } = require(path.join(ROOT, "textSegment.js"));
const { Marker } = require(path.join(ROOT, "mergeTree.js"));
const { LocalReference } = require(path.join(ROOT, "localReference.js"));

const MARKER_KEY = 3;  // the logs' key id of the reserved "markerId" property; "m<v>" is value id v
const SLIDE = 0x40;    // ReferenceType.SlideOnRemove
const F_REWRITE = 1, F_MARKER = 128, OP_INSERT_AT = 5;

function specToSegment(spec) { return TextSegment.fromJSONObject(spec) || Marker.fromJSONObject(spec); }
const logger = { send() {}, sendTelemetryEvent() {}, sendErrorEvent() {}, sendPerformanceEvent() {} };

function rng(seed) {  // xorshift32
    let s = seed >>> 0 || 1;
    return () => {
        s ^= s << 13; s >>>= 0; s ^= s >>> 17; s ^= s << 5; s >>>= 0;
        return s / 4294967296;
    };
}

function keyId(k) { return k === "markerId" ? MARKER_KEY : parseInt(k.slice(1), 10); }
function valId(k, v) { return v === null || v === undefined ? null : k === "markerId" ? parseInt(v.slice(1), 10) : v; }
function propIds(p) {
    if (!p) return null;
    const o = {};
    for (const k of Object.keys(p)) o[keyId(k)] = valId(k, p[k]);
    return o;
}
function record(seq, ref, msn, client, op) {
    if (op.type === 0) {
        const seg = op.seg;
        if (seg.marker) return [seq, ref, msn, client, 0, op.pos1, 0, String.fromCharCode(seg.marker.refType), propIds(seg.props), F_MARKER];
        const text = typeof seg === "string" ? seg : seg.text;
        return [seq, ref, msn, client, 0, op.pos1, 0, text, typeof seg === "string" ? null : propIds(seg.props), 0];
    }
    if (op.type === 1) return [seq, ref, msn, client, 1, op.pos1, op.pos2, null, null, 0];
    return [seq, ref, msn, client, 2, op.pos1, op.pos2, null, propIds(op.props),
        op.combiningOp && op.combiningOp.name === "rewrite" ? F_REWRITE : 0];
}

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

function logId(client, shortId) {
    if (shortId < 0) return -2;
    return parseInt(client.getLongClientId(shortId).slice(1), 10);
}

function canonical(client) {
    const mt = client.mergeTree;
    const segs = [];
    for (const ch of leaves(client)) {
        const removed = ch.removedSeq !== undefined;
        const ov = (ch.removedClientOverlap || []).map((x) => logId(client, x)).sort((a, b) => a - b);
        let props = null;
        if (ch.properties) {
            const ids = propIds(ch.properties);
            props = {};
            for (const k of Object.keys(ids).map((x) => parseInt(x, 10)).sort((a, b) => a - b)) props["k" + k] = ids[k];
        }
        segs.push([Marker.is(ch) ? { marker: ch.refType } : ch.text, ch.seq, logId(client, ch.clientId), removed ? ch.removedSeq : -1,
            removed ? logId(client, ch.removedClientId) : -1, ov, props]);
    }
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

// c1 and what it was handed, in order: {t: "msg", m} | {t: "local", op} | {t: "ref", pos, type} | {t: "at", id, spec}
function makeDoc(name) {
    const c = new Client(specToSegment, logger);
    c.startOrUpdateCollaboration("c1");
    const d = { name, c, items: [], records: [], refs: [], refObjs: [], ats: [], checkpoints: [], ev: null,
        counts: { applied: 0, split: 0, left: 0, moved: 0, differs: 0, first: 0, zero: 0, detached: 0 } };
    const where = (seg) => {
        let ord = 0, pos = 0;
        for (const ch of leaves(c)) {
            if (ch === seg) return [ord, pos];
            ord++;
            pos += ch.removedSeq === undefined ? ch.cachedLength : 0;
        }
        return [-1, -1];
    };
    c.mergeTreeDeltaCallback = (opArgs, args) => {
        if (!d.ev) return;
        d.ev.push([-1, args.operation, args.deltaSegments.map((x) => {
            const [leaf, pos] = where(x.segment);
            return [leaf, pos, x.segment.cachedLength, null];
        })]);
    };
    c.mergeTreeMaintenanceCallback = (args) => {
        if (!d.ev) return;
        const segs = [];
        for (let i = 0; i < args.deltaSegments.length; i++) {
            const seg = args.deltaSegments[i].segment;
            let leaf = where(seg)[0];
            if (args.operation === -2 && i === 1) leaf = segs[0][0] + 1;  // SPLIT: `next` is not linked yet
            segs.push([leaf, -1, seg.cachedLength, null]);
        }
        d.ev.push([-1, args.operation, segs]);
    };
    return d;
}

function step(c, refObjs, it) {
    if (it.t === "msg") c.applyMsg(it.m);
    else if (it.t === "local") {
        const op = it.op;
        if (op.type === 0) c.insertSegmentLocal(op.pos1, specToSegment(op.seg));
        else if (op.type === 1) c.removeRangeLocal(op.pos1, op.pos2);
        else c.annotateRangeLocal(op.pos1, op.pos2, op.props, op.combiningOp);
    } else if (it.t === "ref") {
        const so = c.getContainingSegment(it.pos);
        const ref = new LocalReference(c, so.segment, so.offset, it.type);
        c.addLocalReference(ref);
        refObjs.push(ref);
    } else {
        c.insertAtReferencePositionLocal(refObjs[it.id], specToSegment(it.spec));
    }
}

// the leaves a fresh c1 holds after the same items and then insertSegmentLocal(pos, spec)
function absoluteLeaves(d, pos, spec) {
    const c = new Client(specToSegment, logger);
    c.startOrUpdateCollaboration("c1");
    const refObjs = [];
    for (const it of d.items) step(c, refObjs, it);
    c.insertSegmentLocal(pos, specToSegment(spec));
    return JSON.stringify(canonical(c).segs);
}

function deliver(d, m) {
    d.c.applyMsg(m);
    d.items.push({ t: "msg", m });
    const op = m.contents;
    d.records.push(record(m.sequenceNumber, m.referenceSequenceNumber, m.minimumSequenceNumber, parseInt(m.clientId.slice(1), 10), op));
}
function noteLocal(d, op) {
    d.items.push({ t: "local", op });
    d.records.push(record(-1, 0, 0, 1, op));
}
// false: the reference's addLocalRef threw (localReference.ts:212-219 after a slide) before changing anything
function addRef(d, pos, type) {
    const c = d.c;
    const so = c.getContainingSegment(pos);
    if (!so.segment) return false;
    const ref = new LocalReference(c, so.segment, so.offset, type);
    try {
        c.addLocalReference(ref);
    } catch (e) {
        if (!(e instanceof TypeError)) throw e;
        return false;
    }
    d.refs.push([d.records.length, d.refObjs.length, pos, type]);
    d.refObjs.push(ref);
    d.items.push({ t: "ref", pos, type });
    return true;
}
function refRow(order, r) {
    const p = r.toPosition();
    if (p < 0) return 0;
    return [p, order.indexOf(r.segment), r.getOffset()];
}
// c1.insertAtReferencePositionLocal(reference id, seg): the op, or undefined for a detached reference
function insertAt(d, id, seg, keepState) {
    const c = d.c, ref = d.refObjs[id];
    const spec = seg.toJSONObject();
    const before = leaves(c);
    const linked = ref.segment !== undefined && ref.segment.parent !== undefined;
    const refOrd = linked ? before.indexOf(ref.segment) : -1;
    const refOff = linked ? ref.getOffset() : 0;
    const zero = linked && ref.segment.removedSeq !== undefined;
    const pre = before.map((s) => (s.removedSeq === undefined ? "." : s.removedSeq === -1 ? "p" : "x")).join("");
    const k = d.records.length;
    d.ev = [];
    const op = c.insertAtReferencePositionLocal(ref, seg);
    const ev = d.ev;
    d.ev = null;
    const rec = record(-1, 0, 0, 1, { type: 0, pos1: id, seg: spec });
    rec[4] = OP_INSERT_AT;
    d.records.push(rec);
    if (!op) {
        if (ev.length) throw new Error("a detached insert fired callbacks");
        d.items.push({ t: "at", id, spec });
        d.ats.push({ k, id, op: null });
        d.counts.detached++;
        return undefined;
    }
    const after = leaves(c);
    const ord = after.indexOf(seg);
    const split = ev.some((e) => e[1] === -2);
    const moved = ord < (split ? refOrd + 1 : refOrd);  // the excursion passed leaves without local length
    const left = ord <= refOrd;                         // in front of the reference's segment, not inside it
    const blocks = [];
    for (const s of after) if (!blocks.length || blocks[blocks.length - 1] !== s.parent) blocks.push(s.parent);
    const first = seg.parent.children[0] === seg && blocks[0] !== seg.parent;
    const state = canonical(c);
    const differs = absoluteLeaves(d, op.pos1, spec) !== JSON.stringify(state.segs);
    d.items.push({ t: "at", id, spec });
    const row = { k, id, op: op.pos1, ord, n: after.length, levels: state.tree.map((l) => l.length), split, refOrd, refOff,
        pre, left, moved, zero, first, differs, refs: d.refObjs.map((r) => refRow(after, r)), ev };
    if (keepState) row.state = state;
    d.ats.push(row);
    const n = d.counts;
    n.applied++; n.split += split ? 1 : 0; n.left += left ? 1 : 0; n.moved += moved ? 1 : 0; n.differs += differs ? 1 : 0;
    n.first += first ? 1 : 0; n.zero += zero ? 1 : 0;
    return op;
}
function checkpoint(d) { d.checkpoints.push({ k: d.records.length, state: canonical(d.c) }); }
function finish(d) {
    checkpoint(d);
    return { name: d.name, records: d.records, refs: d.refs, ats: d.ats, checkpoints: d.checkpoints, counts: d.counts, marker: d.marker };
}

// ------------------------------------------------------------------------------------ scenarios
// One scenario: c1 and a hand-driven sequencer.  Remote clients are plain message sources that have
// seen every sequenced message (ref = the sequencer's seq) unless a ref is given; the msn stays 0
// (nothing is zambonied) until msn() moves it.
class Scenario {
    constructor(name) {
        this.d = makeDoc(name);
        this.seq = 0;
        this.minSeq = 0;
        this.pending = [];
    }
    msg(cl, ref, op) {
        this.seq++;
        return { clientId: "c" + cl, clientSequenceNumber: 1, contents: op, metadata: undefined, minimumSequenceNumber: this.minSeq,
            origin: undefined, referenceSequenceNumber: ref, sequenceNumber: this.seq, timestamp: 0, term: 1, traces: [], type: "op" };
    }
    remote(cl, op, ref) { deliver(this.d, this.msg(cl, ref === undefined ? this.seq : ref, op)); }
    rins(cl, pos, text, ref) { this.remote(cl, { type: 0, pos1: pos, seg: text }, ref); }
    rrem(cl, a, b, ref) { this.remote(cl, { type: 1, pos1: a, pos2: b }, ref); }
    // n segments of `w` characters appended by client 2, one message each
    fill(n, w) {
        for (let i = 0; i < n; i++) {
            let t = "";
            for (let q = 0; q < w; q++) t += String.fromCharCode(97 + (i + q) % 26);
            this.rins(2, this.d.c.getLength(), t);
        }
    }
    lins(pos, text) { this.local(this.d.c.insertSegmentLocal(pos, new TextSegment(text))); }
    lrem(a, b) { this.local(this.d.c.removeRangeLocal(a, b)); }
    local(op) {
        if (!op) throw new Error("local op rejected");
        this.pending.push({ op, ref: this.d.c.getCurrentSeq() });
        noteLocal(this.d, op);
    }
    ack(n) {
        const k = n === undefined ? this.pending.length : Math.min(n, this.pending.length);
        for (let i = 0; i < k; i++) {
            const p = this.pending.shift();
            deliver(this.d, this.msg(1, p.ref, p.op));
        }
    }
    ref(pos, type) {
        if (!addRef(this.d, pos, type || 0)) throw new Error("scenario: addLocalReference failed");
        return this.d.refObjs.length - 1;
    }
    at(id, seg) {
        const op = insertAt(this.d, id, typeof seg === "string" ? new TextSegment(seg) : seg, true);
        if (op) this.pending.push({ op, ref: this.d.c.getCurrentSeq() });
        return op;
    }
    last() { return this.d.ats[this.d.ats.length - 1]; }
    expect(cond, what) { if (!cond) throw new Error(`scenario ${this.d.name}: expected ${what}: ${JSON.stringify(Object.assign({}, this.last(), { state: undefined, refs: undefined, pre: undefined }))}`); }
    done() {
        this.ack();
        return finish(this.d);
    }
}

function scenarios() {
    const out = [];
    let s;

    // the reference's segment is the first child of the second leaf block: the new leaf becomes that
    // block's first child (an absolute insert appends to the first block)
    for (const n of [9, 10, 12]) {
        s = new Scenario("block_first_" + n);
        s.fill(n, 2);
        s.at(s.ref(8), "AT");
        s.expect(s.last().ord === 4 && s.last().first && !s.last().split && s.last().differs === false, "first child of block 1, same leaf order");
        s.expect(JSON.stringify(s.last().state.tree) === JSON.stringify(n < 12 ? [[2], [4, n - 3]] : [[3], [4, 5, 4]]), "the second block grows");
        out.push(s.done());
    }

    // a single leaf block: offset 0 on the very first leaf, offset len - 1, offset 1 of 2 characters
    s = new Scenario("single_block");
    s.rins(2, 0, "ab"); s.rins(2, 2, "cde"); s.rins(2, 5, "fg");
    s.at(s.ref(0), "X");
    s.expect(s.last().ord === 0 && !s.last().split, "in front of everything");
    s.at(s.ref(1 + 2 + 2), "Y");   // "cde" offset 2 = len - 1
    s.expect(s.last().split && s.last().refOff === 2, "split at len - 1");
    s.at(s.ref(s.d.c.getLength() - 1), "Z");  // "fg" offset 1
    s.expect(s.last().split && s.last().refOff === 1, "split of a 2-character segment");
    out.push(s.done());

    // a start block with 7 children: one split 4/4
    s = new Scenario("split_block_7");
    s.fill(11, 2);  // leaf blocks [4, 7]
    s.at(s.ref(12), "AT");  // offset 0 of leaf 6, inside block 1
    s.expect(!s.last().split && JSON.stringify(s.last().state.tree) === JSON.stringify([[3], [4, 4, 4]]), "[4,4,4]");
    out.push(s.done());

    // a full block and the offset inside the segment: the split half and the insert in one op, on
    // either side of the block's middle
    for (const leaf of [4, 9]) {
        s = new Scenario("split_half_and_insert_" + leaf);
        s.fill(11, 2);
        s.at(s.ref(2 * leaf + 1), "AT");
        s.expect(s.last().split && s.last().ord === leaf + 1 && s.last().levels[1] === 3, "split half linked, block split");
        out.push(s.done());
    }

    // a root with 7 children whose last block fills: split, root with 8 children, updateRoot
    s = new Scenario("update_root");
    s.fill(31, 2);  // leaf blocks 6 x 4 + 7
    s.at(s.ref(2 * 27), "AT");
    s.expect(s.last().levels.length === 3, "three levels");
    out.push(s.done());

    // a run of pending-removed leaves in front of the reference's segment, longer than a wave and
    // across many blocks: the new leaf goes to the run's far end
    s = new Scenario("pending_run_80");
    s.fill(100, 1);
    { const r = s.ref(90); s.lrem(10, 90); s.at(r, "AT"); }
    s.expect(s.last().ord === 10 && s.last().moved && s.last().refOrd === 90, "ordinal 10");
    out.push(s.done());
    s = new Scenario("pending_run_64");  // exactly one window, the leaf before it live
    s.fill(100, 1);
    { const r = s.ref(74); s.lrem(10, 74); s.at(r, "AT"); }
    s.expect(s.last().ord === 10 && s.last().refOrd === 74, "ordinal 10");
    out.push(s.done());
    s = new Scenario("pending_run_to_front");  // the run reaches the first leaf
    s.fill(100, 1);
    { const r = s.ref(70); s.lrem(0, 70); s.at(r, "AT"); }
    s.expect(s.last().ord === 0, "ordinal 0");
    out.push(s.done());

    // the same run with acked tombstones interleaved (breakTie false for them), one of them the run's
    // far end; then with every removal acked: nothing moves
    s = new Scenario("pending_run_acked_mix");
    s.fill(100, 1);
    {
        const r = s.ref(90);
        for (let i = 0; i < 16; i++) s.rrem(3, 10 + 4 * i, 11 + 4 * i);  // leaves 10, 15, 20, ... removed by c3
        s.lrem(10, 90 - 16);
        s.at(r, "AT");
        s.expect(s.last().ord === 11 && s.last().pre[10] === "x" && s.last().pre[11] === "p", "ordinal 11, behind the acked far end");
        const r2 = s.ref(10);   // the same leaf again, after everything is acked
        s.ack();
        s.at(r2, "ZZ");
        s.expect(!s.last().moved && s.last().pre[s.last().refOrd - 1] === "x", "nothing moves over acked tombstones");
    }
    out.push(s.done());

    // a reference on an acked tombstone: c2, which has not seen c1's pending removal of leaf 5, removes
    // leaf 4 and slides its SlideOnRemove reference onto leaf 5; c1's removal is acked; the insert goes
    // in front of leaf 5, where a walk from the root would pass it
    s = new Scenario("ref_on_acked_tombstone");
    s.fill(10, 2);
    {
        const r = s.ref(8, SLIDE);
        const seen = s.seq;
        s.lrem(10, 12);
        s.rrem(2, 8, 10, seen);
        s.ack();
        s.at(r, "AT");
        s.expect(s.last().zero && s.last().pre[s.last().refOrd] === "x" && s.last().ord === s.last().refOrd && s.last().differs,
            "in front of the acked tombstone, unlike an absolute insert");
    }
    out.push(s.done());

    // a reference kept on its removed segment by the clear() quirk: everything is removed while the
    // reference sits in an `after` list
    s = new Scenario("ref_kept_by_clear");
    s.fill(3, 2);
    {
        const r = s.ref(2, SLIDE);       // on "bc"
        s.rrem(2, 2, 6);                  // slides after tombstones: onto "ab", offset 1, an `after` list
        s.rrem(2, 0, 2);                  // nothing left: clear() keeps it
        s.at(r, "AT");
        if (s.last().op !== null) s.expect(s.last().zero, "on a removed segment");
    }
    out.push(s.done());

    // a detached reference: nothing happens
    s = new Scenario("detached");
    s.fill(5, 2);
    {
        const r = s.ref(4);
        s.rrem(2, 4, 6);
        s.at(r, "AT");
        s.expect(s.last().op === null, "undefined");
        s.at(s.ref(1), "OK");
        s.expect(s.last().op === 1 && s.last().split, "the next one applies");
    }
    out.push(s.done());

    // a marker with a markerId at a reference, then posFromRelativePos on it
    s = new Scenario("marker_with_id");
    s.fill(6, 2);
    {
        const r = s.ref(5);
        s.lrem(2, 4);
        const mk = new Marker(1);
        mk.addProperties({ markerId: "m7" });
        s.at(r, mk);
        s.expect(s.last().split && s.last().op === 3, "split, pos 3");
        s.d.marker = { id: 7, key: MARKER_KEY, k: s.d.records.length,
            before: s.d.c.posFromRelativePos({ id: "m7", before: true }), after: s.d.c.posFromRelativePos({ id: "m7" }) };
        s.at(s.ref(0), "P");
    }
    out.push(s.done());

    // every editing form: the LDS form at 256 / 512 / 1024 slots, the workspace form at 2048 with a
    // document past 1,024 segments; in each a split, a pending run across blocks and a block split
    for (const n of [150, 330, 700, 1100]) {
        s = new Scenario("form_" + n);
        s.fill(n, 2);
        const a = s.ref(2 * (n - 20) + 1), b = s.ref(2 * (n >> 1));
        s.lrem(2 * (n >> 1) - 140, 2 * (n >> 1));
        s.at(b, "MID");
        s.expect(s.last().moved && s.last().ord === (n >> 1) - 70, "over 70 pending leaves");
        s.at(a, "END");
        s.expect(s.last().split, "split");
        out.push(s.done());
    }

    // more than 64 edits pending when the insert arrives: the four-word group-mask form
    s = new Scenario("groups_70");
    s.fill(40, 2);
    {
        const r = s.ref(41);
        for (let i = 0; i < 70; i++) s.lins((7 * i) % s.d.c.getLength(), "q");
        s.lrem(30, 34);
        s.at(r, "AT");
        s.expect(s.pending.length > 64 && s.last().op !== null, "71 edits pending");
        s.ack(30);
        s.at(r, "A2");
    }
    out.push(s.done());
    return out;
}

// ----------------------------------------------------------------------------------------- farm
// oracle/tsref/local_farm.js's farm (4 clients behind a toy sequencer, rounds, c1 lagging with `partial`),
// with c1 holding local references and making 30 % of its edits at one of them.  null: the clients
// diverged or one threw.
function farm(seed, nOps, nClients, partial) {
    const r = rng(seed);
    const ri = (n) => Math.floor(r() * n);
    const d = makeDoc("run" + seed);
    const clients = [d.c];
    for (let i = 2; i <= nClients; i++) {
        const c = new Client(specToSegment, logger);
        c.startOrUpdateCollaboration("c" + i);
        clients.push(c);
    }
    const queue = [], seqd = [];
    const cursor = clients.map(() => 0);
    let seq = 0, made = 0;
    const marks = [];
    for (let q = 1; q <= 4; q++) marks.push(Math.floor(nOps * q / 5));
    const deliverTo = (i) => {
        const m = seqd[cursor[i]++];
        if (i === 0) deliver(d, m); else clients[i].applyMsg(m);
    };
    const randomSeg = () => {
        const n = 1 + ri(4);
        let text = "";
        for (let q = 0; q < n; q++) text += String.fromCharCode(97 + ri(26));
        const seg = new TextSegment(text);
        if (r() < 0.25) { const props = {}; props["k" + ri(3)] = 1 + ri(4); seg.addProperties(props); }
        return seg;
    };
    const localOp = (i) => {
        const c = clients[i];
        made++;
        if (i === 0) {
            if (d.refObjs.length < 24 && c.getLength() > 0 && r() < 0.3) addRef(d, ri(c.getLength()), d.refObjs.length % 2 ? SLIDE : 0);
            if (d.refObjs.length && r() < 0.3) {
                const op = insertAt(d, ri(d.refObjs.length), randomSeg(), false);
                if (op) queue.push({ client: 1, ref: c.getCurrentSeq(), op });
                if (marks.length && made >= marks[0]) { marks.shift(); checkpoint(d); }
                return;
            }
        }
        const len = c.getLength();
        const pick = r();
        let op;
        if (len === 0 || pick < 0.45) {
            op = c.insertSegmentLocal(ri(len + 1), randomSeg());
        } else {
            const a = ri(len), b = a + 1 + ri(Math.min(6, len - a));
            if (pick < 0.75) {
                op = c.removeRangeLocal(a, b);
            } else {
                const props = {};
                const nk = 1 + ri(2);
                for (let q = 0; q < nk; q++) props["k" + ri(3)] = r() < 0.15 ? null : 1 + ri(4);
                op = c.annotateRangeLocal(a, b, props, r() < 0.1 ? { name: "rewrite" } : undefined);
            }
        }
        if (!op) throw new Error("local op rejected");
        queue.push({ client: i + 1, ref: c.getCurrentSeq(), op });
        if (i === 0) {
            noteLocal(d, op);
            if (marks.length && made >= marks[0]) { marks.shift(); checkpoint(d); }
        }
    };
    const sequenceAll = () => {
        while (queue.length) {
            const q = queue.shift();
            seq++;
            const msn = Math.min(q.ref, ...clients.map((c) => c.getCurrentSeq()), ...queue.map((o) => o.ref));
            seqd.push({ clientId: "c" + q.client, clientSequenceNumber: 1, contents: q.op, metadata: undefined,
                minimumSequenceNumber: msn, origin: undefined, referenceSequenceNumber: q.ref, sequenceNumber: seq,
                timestamp: 0, term: 1, traces: [], type: "op" });
        }
    };
    while (made < nOps) {
        for (let i = 0; i < nClients; i++) {
            const k = r() < 0.6 ? 1 + ri(3) : 0;
            for (let q = 0; q < k; q++) localOp(i);
        }
        sequenceAll();
        for (let i = 1; i < nClients; i++) while (cursor[i] < seqd.length) deliverTo(i);
        const upto = partial ? cursor[0] + ri(seqd.length - cursor[0] + 1) : seqd.length;
        while (cursor[0] < upto) deliverTo(0);
    }
    while (cursor[0] < seqd.length) deliverTo(0);
    const txt = (c) => c.createTextHelper().getText(c.getCurrentSeq(), c.getClientId());
    const t0 = txt(clients[0]);
    for (const c of clients) if (txt(c) !== t0) return null;
    return finish(d);
}

const mode = process.argv[2];
if (mode === "scenarios") {
    process.stdout.write(scenarios().map((x) => JSON.stringify(x)).join("\n") + "\n");
} else if (mode === "farm") {
    const [seed, runs, nOps, partial] = process.argv.slice(3).map((x) => parseInt(x, 10));
    let dropped = 0;
    for (let k = 0; k < runs; k++) {
        let doc = null;
        try {
            doc = farm(seed * 7919 + k, nOps, 4, partial === 1);
        } catch (err) {
            if (process.env.FARM_DEBUG) process.stderr.write(`refinsert farm: run ${k}: ${err.stack}\n`);
        }
        if (doc) process.stdout.write(JSON.stringify(doc) + "\n"); else dropped++;
    }
    process.stdout.write(JSON.stringify({ dropped, tried: runs }) + "\n");
} else {
    throw new Error("usage: refinsert_ref.js scenarios | farm <seed> <runs> <ops> <lag>");
}
