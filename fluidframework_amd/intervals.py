"""Interval collections of the batched engine (include/mtgpu.h "interval collections").

A `SequenceInterval` (packages/dds/sequence/src/intervalCollection.ts:107-190) is two local
references; the engine keeps a document's intervals on the device as pairs of handles into its
reference table and answers `findOverlappingIntervals` with the reference's own per-interval
predicate.  This module holds the record layouts of `MergeEngine.add_intervals / remove_intervals /
overlapping_intervals / interval_positions` and, in plain Python, the rules themselves: `compare`
and `overlaps` on endpoints given as (segment ordinal | None, raw offset).
"""
import numpy as np

# mt_interval_add: addInterval(start, end, intervalType)
INTERVAL_ADD_DTYPE = np.dtype([('doc', '<u4'), ('start', '<i4'), ('end', '<i4'), ('interval_type', '<u2'), ('collection', '<u2')])
# mt_interval_query: the transient interval of findOverlappingIntervals / removeInterval
INTERVAL_QUERY_DTYPE = np.dtype([('doc', '<u4'), ('start', '<i4'), ('end', '<i4'), ('collection', '<u4')])
# mt_interval_pos: toPosition() of both ends (-1 detached), the intervalType, its collection's id, live, and
# the two ends' reference handles (MergeEngine.ref_positions)
INTERVAL_POS_DTYPE = np.dtype([('start', '<i4'), ('end', '<i4'), ('interval_type', '<u2'), ('collection', '<u2'),
                               ('live', '<u4'), ('start_ref', '<u4'), ('end_ref', '<u4')])
assert INTERVAL_ADD_DTYPE.itemsize == 16 and INTERVAL_QUERY_DTYPE.itemsize == 16 and INTERVAL_POS_DTYPE.itemsize == 24

INTERVAL_SIMPLE = 0x0           # IntervalType (ops.ts:17-22)
INTERVAL_NEST = 0x1
INTERVAL_SLIDE_ON_REMOVE = 0x2


def ref_types(interval_type):
    """(start, end) ReferenceType of an interval's two references (createSequenceInterval,
    intervalCollection.ts:207-228): RangeBegin / RangeEnd, NestBegin / NestEnd when the type is exactly
    Nest, each with SlideOnRemove when the type has it."""
    begin, end = (0x2, 0x4) if interval_type == INTERVAL_NEST else (0x10, 0x20)
    if interval_type & INTERVAL_SLIDE_ON_REMOVE:
        begin, end = begin | 0x40, end | 0x40
    return begin, end


def compare(a, b):
    """LocalReference.compare (localReference.ts:49-61) on (ordinal | None, offset): the same segment,
    or both without one, by raw offset; one without a segment sorts below every segment; else the
    order of the segments among the leaves."""
    if a[0] == b[0]:
        return a[1] - b[1]
    if a[0] is None:
        return -1
    if b[0] is None:
        return 1
    return -1 if a[0] < b[0] else 1


def overlaps(interval, query):
    """SequenceInterval.overlaps (intervalCollection.ts:149-156); both arguments (start, end)."""
    return compare(interval[0], query[1]) < 0 and compare(interval[1], query[0]) >= 0


def equal(interval, query):
    """SequenceInterval.compare(...) == 0 (intervalCollection.ts:140-147): what removeInterval looks for."""
    return compare(interval[0], query[0]) == 0 and compare(interval[1], query[1]) == 0
