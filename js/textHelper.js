"use strict";
// textHelper.js -- MergeTreeTextHelper (packages/dds/merge-tree/src/textSegment.ts:124-276) over the
// engine's batched text read (include/mtgpu.h "text reads", N-API textRanges): getText and
// getTextAndMarkers of one BatchClient's document, in any view.
//
// The device gathers the text (mapRange -> nodeMap with gatherText as the leaf action) and lists the
// visited markers as {ordinal, out_offset}; what the reference builds from Marker objects is composed
// here: the "*" placeholder ("\n" + marker.toString() at each marker, mergeTree.ts:723-787) and
// getTextAndMarkers' cut at the markers that hold the label (Marker.hasTileLabel, mergeTree.ts:581-597),
// from each marker's refType and properties read by ordinal (mt_segment_infos).  gatherText also wraps
// runs in <b> / <u> by the segments' "font-weight" / "text-decoration" properties in parallel-array
// mode: a document that has interned either key is answered through BatchClient.walkSegments on the
// host (the local view only), so the result stays exact.
const TEXT_MARKERS = 1, POS_LOCAL = -2147483648, QUERY = 32, INT32_MAX = 2147483647;
const TILE_LABELS = "referenceTileLabels", RANGE_LABELS = "referenceRangeLabels";
const TILE = 1, NEST_BEGIN = 2, NEST_END = 4;  // ReferenceType (ops.ts:6-16)

const hasTileLabels = (m) => (m.refType & TILE) && m.properties && m.properties[TILE_LABELS];
const hasRangeLabels = (m) => (m.refType & (NEST_BEGIN | NEST_END)) && m.properties && m.properties[RANGE_LABELS];

/** Marker.toString (mergeTree.ts:723-787) of a marker descriptor {refType, properties} */
function markerToString(m) {
    let bbuf = "";
    if (m.refType & TILE) bbuf += "Tile";
    if (m.refType & NEST_BEGIN) bbuf += (bbuf.length > 0 ? "; " : "") + "RangeBegin";
    if (m.refType & NEST_END) bbuf += (bbuf.length > 0 ? "; " : "") + "RangeEnd";
    const id = m.properties && m.properties.markerId;
    if (id) bbuf += ` (${id}) `;
    let lbuf = "";
    if (hasTileLabels(m)) lbuf += "tile -- " + m.properties[TILE_LABELS].join("; ");
    if (hasRangeLabels(m)) {
        if (hasTileLabels(m)) lbuf += " ";
        lbuf += `range ${m.refType & NEST_END ? "end" : "begin"} -- ` + m.properties[RANGE_LABELS].join("; ");
    }
    const pbuf = m.properties ? JSON.stringify(m.properties) : "";
    return `M ${bbuf}: ${lbuf} ${pbuf}`;
}

class TextHelper {
    constructor(client) { this.client = client; }

    // one read: {text, markers: [{ordinal, offset}]}; the defaults of start / end are the host's
    _read(refSeq, clientId, placeholder, start, end, wantMarkers) {
        const c = this.client;
        c.engine.flush();
        c._checkError();
        const local = clientId === c.getClientId() && refSeq === c.getCurrentSeq();  // the client's own view
        const q = Buffer.alloc(QUERY);
        q.writeUInt32LE(c.doc, 0);
        q.writeInt32LE(start === undefined ? 0 : start, 4);
        q.writeInt32LE(end === undefined ? INT32_MAX : end, 8);
        q.writeInt32LE(local ? POS_LOCAL : refSeq, 12);
        q.writeUInt16LE(local ? 0 : clientId, 16);
        q.writeUInt16LE(placeholder ? placeholder.charCodeAt(0) : 0, 18);
        q.writeUInt32LE(wantMarkers ? TEXT_MARKERS : 0, 20);
        const [units, rp, marks, mrp] = c.engine.native.textRanges(c.engine.handle, q);
        const text = units.toString("utf16le", 0, 2 * rp.readUInt32LE(4));
        const markers = [];
        for (let i = 0; i < mrp.readUInt32LE(4); i++) markers.push({ ordinal: marks.readInt32LE(8 * i), offset: marks.readUInt32LE(8 * i + 4) });
        return { text, markers };
    }

    /** MergeTreeTextHelper.getText (textSegment.ts:154-172) */
    getText(refSeq, clientId, placeholder = "", start, end) {
        if (placeholder.length > 1) throw new Error("TextHelper.getText: a placeholder is one UTF-16 unit");
        if (placeholder !== "*") return this._read(refSeq, clientId, placeholder, start, end, false).text;
        const r = this._read(refSeq, clientId, "", start, end, true);
        let out = "", at = 0;
        for (const m of r.markers) {
            out += r.text.slice(at, m.offset) + "\n" + markerToString(this.client._descriptorAt(m.ordinal));
            at = m.offset;
        }
        return out + r.text.slice(at);
    }

    /** MergeTreeTextHelper.getTextAndMarkers (textSegment.ts:127-152): markers as segment descriptors */
    getTextAndMarkers(refSeq, clientId, label, start, end) {
        const c = this.client;
        if (c.keyIds.has("font-weight") || c.keyIds.has("text-decoration")) return this._taggedOnHost(refSeq, clientId, label, start, end);
        const r = this._read(refSeq, clientId, "", start, end, true);
        const parallelText = [], parallelMarkers = [];
        let at = 0;
        for (const m of r.markers) {
            const d = c._descriptorAt(m.ordinal);
            if (hasTileLabels(d) && d.properties[TILE_LABELS].includes(label)) {
                parallelMarkers.push(d);
                parallelText.push(r.text.slice(at, m.offset));
                at = m.offset;
            }
        }
        return { parallelText, parallelMarkers };
    }

    // gatherText's parallel-array mode with its tags (textSegment.ts:196-253, 264-271) over walkSegments
    _taggedOnHost(refSeq, clientId, label, start, end) {
        const c = this.client;
        if (clientId !== c.getClientId() || refSeq !== c.getCurrentSeq()) {
            throw new Error("TextHelper.getTextAndMarkers: a document with font-weight / text-decoration is read in the local view only");
        }
        const parallelText = [], parallelMarkers = [], inProgress = [];
        let text = "";
        c.walkSegments((seg, pos, rs, cl, s, e) => {
            if (seg.refType !== undefined) {
                if (hasTileLabels(seg) && seg.properties[TILE_LABELS].includes(label)) {
                    parallelMarkers.push(seg);
                    parallelText.push(text);
                    text = "";
                }
                return true;
            }
            const tags = [], init = [], rem = [];
            let beginTags = "", endTags = "";
            if (seg.properties && seg.properties["font-weight"]) tags.push("b");
            if (seg.properties && seg.properties["text-decoration"]) tags.push("u");
            if (tags.length > 0) {
                for (const t of tags) if (!inProgress.includes(t)) { beginTags += `<${t}>`; init.push(t); }
                for (const t of inProgress) if (!tags.includes(t)) { endTags += `</${t}>`; rem.push(t); }
                for (const t of init.reverse()) inProgress.push(t);
            } else {
                for (const t of inProgress) { endTags += `</${t}>`; rem.push(t); }
            }
            for (const t of rem) { const i = inProgress.indexOf(t); if (i >= 0) inProgress.splice(i, 1); }
            text += endTags + beginTags;
            if (s <= 0 && e >= seg.text.length) text += seg.text;
            else text += e >= seg.text.length ? seg.text.substring(Math.max(s, 0)) : seg.text.substring(Math.max(s, 0), e);
            return true;
        }, start, end);
        return { parallelText, parallelMarkers };
    }
}

module.exports = { TextHelper, markerToString };
