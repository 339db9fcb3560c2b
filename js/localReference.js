"use strict";
// localReference.js -- LocalReference (packages/dds/merge-tree/src/localReference.ts:20-119) over the
// device's reference table (include/mtgpu.h "local references").  The (segment, offset) pair lives on
// the device and follows the segment through edits there; this object holds its handle, its refType
// and -- host only -- its properties.  Reads flush the engine's queued ops first, as every read of
// BatchClient does.
const ReferenceType = { Simple: 0x0, Tile: 0x1, NestBegin: 0x2, NestEnd: 0x4, RangeBegin: 0x10, RangeEnd: 0x20,
    SlideOnRemove: 0x40, Transient: 0x100 };
const REF_NONE = 0xffffffff, REF_FULL = 0xfffffffe;

class LocalReference {
    /** As the reference's constructor: a segment descriptor of `client` (getContainingSegment) and an
     * offset in it; client.addLocalReference(ref) puts it on the device. */
    constructor(client, segment, offset = 0, refType = ReferenceType.Simple) {
        this.client = client;
        this.refType = refType;
        this.properties = undefined;
        this.handle = undefined;  // set by addLocalReference
        this._at = segment ? { segment, offset } : undefined;
    }

    /** {position, ordinal, offset} now (position / ordinal -1: detached) */
    _query() {
        if (this.handle === undefined) return { position: LocalReference.DetachedPosition, ordinal: -1, offset: 0 };
        return this.client._refPositions([this.handle])[0];
    }
    toPosition() { return this._query().position; }
    getOffset() { return this._query().offset; }
    /** the segment it sits on as a descriptor (valid until the document next changes), or undefined */
    getSegment() {
        const q = this._query();
        if (q.ordinal < 0) return undefined;
        return this.client._descriptorAt(q.ordinal);
    }
    get segment() { return this.getSegment(); }
    get offset() { return this.handle === undefined && this._at ? this._at.offset : this._query().offset; }

    /** document order: by segment, then offset; a detached reference sorts first (localReference.ts:49-61) */
    compare(b) {
        const [x, y] = this.client === b.client && this.handle !== undefined && b.handle !== undefined
            ? this.client._refPositions([this.handle, b.handle]) : [this._query(), b._query()];
        if (x.ordinal === y.ordinal) return x.ordinal < 0 ? 0 : x.offset - y.offset;
        return x.ordinal < 0 || (y.ordinal >= 0 && x.ordinal < y.ordinal) ? -1 : 1;
    }
    min(b) { return this.compare(b) < 0 ? this : b; }
    max(b) { return this.compare(b) > 0 ? this : b; }

    isLeaf() { return false; }
    getProperties() { return this.properties; }
    /** properties.ts addProperties without a combining op (a null value deletes the key) */
    addProperties(newProps, op) {
        if (op) throw new Error("LocalReference.addProperties: combining ops are not supported");
        if (!this.properties) this.properties = {};
        for (const k of Object.keys(newProps)) {
            if (newProps[k] === null) delete this.properties[k]; else this.properties[k] = newProps[k];
        }
    }
}
LocalReference.DetachedPosition = -1;

module.exports = { LocalReference, ReferenceType, REF_NONE, REF_FULL };
