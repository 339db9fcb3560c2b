// mt_marker.h -- which marker an id names, and the position a relative end takes from it
// (include/mtgpu.h "marker-relative positions"): the one rule shared by the apply engine
// (mt_apply.hip rel_lower, over a document staged in LDS or its workspace) and the query kernel
// (mt_markers.hip, over the compact state in HBM).
//
// The reference keeps a map id -> Marker (MergeTree.idToSegment, mergeTree.ts:279-283), filled when a
// marker with a "markerId" property is inserted or loaded and never updated; posFromRelativePos
// (mergeTree.ts:1943-1966) takes getPosition(marker, refSeq, clientId) and steps over the marker or
// back from it.  Here the candidates are the linked Markers -- tombstones too -- whose current value
// of the key is the id; the one inserted last wins: the greatest insert seq, a pending local insert
// (seq -1) above every sequenced one, and among equals the last in document order.
#pragma once
#include <stdint.h>

#include "../../include/mtgpu.h"
#include "mt_wave.h"

#define MT_MARKER_NO_RANK INT32_MIN  // no candidate (a sequenced seq is >= 0)

// a candidate's rank from its insert seq
MT_DEV int32_t mt_marker_rank(int32_t seq) { return seq == -1 ? INT32_MAX : seq; }

// A lane's best candidate so far, folded over its leaves in ascending ordinal: an equal rank at a
// later ordinal replaces the earlier one.
struct mt_marker_best {
    int32_t rank = MT_MARKER_NO_RANK;
    int32_t ord = -1;
    MT_DEV void fold(bool candidate, int32_t seq, int32_t ordinal) {
        if (candidate && mt_marker_rank(seq) >= rank) {
            rank = mt_marker_rank(seq);
            ord = ordinal;
        }
    }
};
// the wave's choice among its lanes' bests: the ordinal, -1 without a candidate (uniform)
MT_DEV int32_t mt_marker_pick(const mt_marker_best& b) {
    const int32_t top = wave_max(b.rank);
    if (top == MT_MARKER_NO_RANK) return -1;
    return wave_max(b.rank == top ? b.ord : -1);
}

// one relative end's block at the payload's tail
struct mt_rel_end {
    uint32_t key;     // the document's key id of "markerId"
    uint32_t value;   // the id string's value id under that key; 0 names no marker
    bool before;
    int32_t offset;
};
MT_DEV mt_rel_end mt_rel_decode(const uint8_t* p) {
    mt_rel_end r;
    r.key = p[0];
    r.before = (p[1] & MT_REL_BEFORE) != 0;
    r.value = (uint32_t)p[2] | ((uint32_t)p[3] << 8);
    r.offset = (int32_t)((uint32_t)p[4] | ((uint32_t)p[5] << 8) | ((uint32_t)p[6] << 16) | ((uint32_t)p[7] << 24));
    return r;
}
// The end's position from the marker's (prefix: the view lengths of the leaves before it; len: its
// cachedLength, 1), clamped to int32: below 0 stays below 0, which the apply refuses.
MT_DEV int32_t mt_rel_position(int32_t prefix, uint32_t len, bool before, int32_t offset) {
    const int64_t p = before ? (int64_t)prefix - offset : (int64_t)prefix + len + offset;
    return p < INT32_MIN ? INT32_MIN : p > INT32_MAX ? INT32_MAX : (int32_t)p;
}
