"use strict";
// intervalCollection.js -- SharedString.getIntervalCollection(label): the reference's
// IntervalCollectionView surface (packages/dds/sequence/src/intervalCollection.ts:514-671) and its
// SequenceInterval (:107-190) over the device's interval table (include/mtgpu.h "interval
// collections").  An interval's two ends are LocalReference objects (localReference.js) on handles of
// the document's reference table; the pair, its intervalType and its collection live on the device.
// Labels, properties and events live here, on the host.  findOverlappingIntervals answers the
// reference's per-interval predicate (SequenceInterval.overlaps on the ends' current segments and raw
// offsets), not the shape of its stale tree; map / serializeInternal go in handle order, not the
// tree's; previousInterval / nextInterval are not offered (INTEGRATION.md).
const { EventEmitter } = require("events");
const path = require("path");
const { LocalReference, ReferenceType, REF_NONE, REF_FULL } = require(path.join(__dirname, "localReference.js"));

const IntervalType = { Simple: 0x0, Nest: 0x1, SlideOnRemove: 0x2, Transient: 0x4 };
const reservedRangeLabelsKey = "referenceRangeLabels";

// properties.ts addProperties without a combining op (a null value deletes the key)
function addProps(old, add) {
    const out = old || {};
    if (add) for (const k of Object.keys(add)) { if (add[k] === null) delete out[k]; else out[k] = add[k]; }
    return out;
}

// createSequenceInterval's reference types (intervalCollection.ts:207-228)
function refTypes(intervalType) {
    let begin = ReferenceType.RangeBegin, end = ReferenceType.RangeEnd;
    if (intervalType === IntervalType.Nest) { begin = ReferenceType.NestBegin; end = ReferenceType.NestEnd; }
    if (intervalType & IntervalType.SlideOnRemove) { begin |= ReferenceType.SlideOnRemove; end |= ReferenceType.SlideOnRemove; }
    return [begin, end];
}

class SequenceInterval {
    constructor(start, end, intervalType, props) {
        this.start = start;
        this.end = end;
        this.intervalType = intervalType;
        this.properties = undefined;
        this.handle = undefined;  // its entry of the document's interval table
        if (props) this.addProperties(props);
    }
    serialize(client) {
        const [s, e] = client._refPositions([this.start.handle, this.end.handle]);
        return this._serialized(client, s.position, e.position);
    }
    _serialized(client, start, end) {
        const out = { end, intervalType: this.intervalType, sequenceNumber: client.getCurrentSeq(), start };
        if (this.properties) out.properties = this.properties;
        return out;
    }
    compare(b) { return this.start.compare(b.start) || this.end.compare(b.end); }
    addProperties(newProps, op) {
        if (op) throw new Error("SequenceInterval.addProperties: combining ops are not supported");
        this.properties = addProps(this.properties, newProps);
    }
    getProperties() { return this.properties; }
}

class IntervalCollection extends EventEmitter {
    /** `id`: the collection's id in its document's table; `emitter` (optional): the value type's op
     * emitter -- emit("add" | "delete", undefined, serializedInterval) for local changes */
    constructor(client, label, id, emitter) {
        super();
        this.client = client;
        this.label = label;
        this.id = id;
        this.emitter = emitter;
        this.intervals = new Map();  // handle -> SequenceInterval
    }

    _query(start, end) {
        const q = Buffer.alloc(16);
        q.writeUInt32LE(this.client.doc, 0);
        q.writeInt32LE(start, 4);
        q.writeInt32LE(end, 8);
        q.writeUInt32LE(this.id, 12);
        return q;
    }
    _ready() {
        this.client.engine._enableIntervals();
        this.client.engine.flush();
        this.client._checkError();
    }

    add(start, end, intervalType, props) {
        const serializedInterval = { end, intervalType, properties: props, sequenceNumber: this.client.getCurrentSeq(), start };
        this.addInternal(serializedInterval, true, undefined);
    }
    delete(start, end) {
        const serializedInterval = { start, end, sequenceNumber: this.client.getCurrentSeq(), intervalType: IntervalType.Transient };
        this.deleteInterval(serializedInterval, true, undefined);
    }

    /** LocalIntervalCollection.addInterval + the view's addInternal (intervalCollection.ts:343-358, 610-631) */
    addInternal(serializedInterval, local, op) {
        this._ready();
        const type = serializedInterval.intervalType || 0;
        const a = this._query(serializedInterval.start, serializedInterval.end);
        a.writeUInt16LE(type & 0xffff, 12);
        a.writeUInt16LE(this.id, 14);
        const native = this.client.engine.native;
        const h = native.intervalsAdd(this.client.engine.handle, a).readUInt32LE(0);
        if (h === REF_FULL || h === REF_NONE) {
            throw new Error("BatchClient: the document's interval or local-reference table is full (intervalsPerDoc, refsPerDoc)");
        }
        const [, refs] = this.client._intervalPositions();
        const [beginType, endType] = refTypes(type);
        const rangeProp = { [reservedRangeLabelsKey]: [this.label] };
        const mk = (handle, refType) => {
            const ref = new LocalReference(this.client, undefined, 0, refType);
            ref.handle = handle;
            ref.addProperties(rangeProp);
            return ref;
        };
        const startRef = mk(refs[h].startRef, beginType), endRef = mk(refs[h].endRef, endType);
        startRef.pairedRef = endRef;
        endRef.pairedRef = startRef;
        const interval = new SequenceInterval(startRef, endRef, type, rangeProp);
        interval.handle = h;
        interval.addProperties(serializedInterval.properties);
        if (this.label && this.label.length > 0) interval.properties[reservedRangeLabelsKey] = [this.label];
        this.intervals.set(h, interval);
        if (local) {
            if (this.emitter) this.emitter.emit("add", undefined, serializedInterval);
        } else if (this.onDeserialize) {
            this.onDeserialize(interval);
        }
        this.emit("addInterval", interval, local, op);
        return this;
    }

    /** removeInterval + the view's deleteInterval (:330-336, 633-650).  The event carries the interval
     * removed, or undefined where none compared equal (the reference hands out its transient interval). */
    deleteInterval(serializedInterval, local, op) {
        this._ready();
        const native = this.client.engine.native;
        const h = native.intervalsRemove(this.client.engine.handle,
            this._query(serializedInterval.start, serializedInterval.end)).readUInt32LE(0);
        const interval = h === REF_NONE ? undefined : this.intervals.get(h);
        if (interval) {
            this.intervals.delete(h);
            interval.handle = undefined;  // (its two references stay, as the reference's do)
        }
        if (local) {
            if (this.emitter) this.emitter.emit("delete", undefined, serializedInterval);
        } else if (this.onDeserialize && interval) {
            this.onDeserialize(interval);
        }
        this.emit("deleteInterval", interval, local, op);
        return this;
    }

    findOverlappingIntervals(startPosition, endPosition) {
        if (this.intervals.size === 0) return [];
        this._ready();
        const [hs, rp] = this.client.engine.native.intervalsOverlapping(this.client.engine.handle,
            this._query(startPosition, endPosition));
        const n = rp.readUInt32LE(4);
        const out = [];
        for (let i = 0; i < n; i++) out.push(this.intervals.get(hs.readUInt32LE(4 * i)));
        return out;
    }

    map(fn) { for (const h of [...this.intervals.keys()].sort((a, b) => a - b)) fn(this.intervals.get(h)); }

    /** every interval's serialize(), with one device call */
    serializeInternal() {
        if (this.intervals.size === 0) return [];
        this._ready();
        const [pos] = this.client._intervalPositions();
        const out = [];
        this.map((iv) => out.push(iv._serialized(this.client, pos[iv.handle].start, pos[iv.handle].end)));
        return out;
    }

    attachDeserializer(onDeserialize) {
        if (!onDeserialize) return;
        this.onDeserialize = onDeserialize;
        this.map((iv) => onDeserialize(iv));
    }
    async getView(onDeserialize) { this.attachDeserializer(onDeserialize); return this; }
    get attached() { return true; }
}

module.exports = { IntervalCollection, SequenceInterval, IntervalType, reservedRangeLabelsKey, refTypes };
