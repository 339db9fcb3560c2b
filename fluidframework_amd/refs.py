"""Local references of the batched engine (include/mtgpu.h "local references").

A `LocalReference` (packages/dds/merge-tree/src/localReference.ts:20-119) is a (segment, offset)
pair that follows its segment through edits; the engine keeps them per document on the device and
moves them by folding the document's delta / maintenance events.  This module holds the record
layouts of `MergeEngine.add_refs / remove_refs / ref_positions`.
"""
import numpy as np

# mt_ref_add: new LocalReference at getContainingSegment(pos) of the local view
REF_ADD_DTYPE = np.dtype([('doc', '<u4'), ('pos', '<i4'), ('ref_type', '<u4')])
# mt_ref_pos: toPosition() (-1 detached), the segment's leaf ordinal (-1 detached), getOffset()
REF_POS_DTYPE = np.dtype([('position', '<i4'), ('ordinal', '<i4'), ('offset', '<u4')])
# mt_ref_insert: the document and reference of one insertAtReferencePositionLocal
REF_INSERT_DTYPE = np.dtype([('doc', '<u4'), ('handle', '<u4')])
assert REF_ADD_DTYPE.itemsize == 12 and REF_POS_DTYPE.itemsize == 12 and REF_INSERT_DTYPE.itemsize == 8

REF_SIMPLE = 0x0            # ReferenceType.Simple (ops.ts:7)
REF_SLIDE_ON_REMOVE = 0x40  # ReferenceType.SlideOnRemove (ops.ts:13)
REF_NONE = 0xFFFFFFFF       # add: pos is outside the local view
REF_FULL = 0xFFFFFFFE       # add: the document's table is full
REF_BAD_HANDLE = -2         # positions: ordinal of a handle that names no reference
DETACHED = -1               # LocalReference.DetachedPosition


def slide_target(pad2):
    """(ordinal | -1, cachedLength, after form) of a REMOVE callback's first row (mt_event.pad2)."""
    t = int(pad2)
    return (t & 0xFFFFFFFF) - 1, (t >> 32) & 0x7FFFFFFF, t >> 63
