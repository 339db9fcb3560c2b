"""Where `Client.insertAtReferencePositionLocal` puts its segment, stated over a canonical state.

The reference (packages/dds/merge-tree/src/client.ts:216-247 -> MergeTree.insertAtReferencePosition,
mergeTree.ts:2000-2097) does not walk from the root for this op.  It starts at the reference's segment:

1. `refOffset !== 0 && refSegLen !== 0` (the segment's length in the local view): the segment is split
   at the offset and the right half becomes the start segment (:2047-2053);
2. `leftExcursion` (:2054-2068, 2280-2310) visits the leaves in front of the start segment, nearest
   first, while their local length is 0; each one `breakTie(0, 0, leaf, currentSeq, own)` holds for
   (:2248-2277: not removed, or its removal still pending) becomes the start segment;
3. the new segment is linked at the start segment's index in the start segment's own block (:2081),
   and the blocks on the way up split as they fill (rebalanceTree, :2010-2040).

The engine's `op_insert_at` (csrc/mt_apply.hip) does the same on the device for an MT_OP_INSERT_AT record
(include/mtgpu.h "local references"); `MergeEngine.insert_at_refs` resolves the reference and lowers the
record in one call.  This module restates the leaf order only; the block shape follows from 3.

A canonical segment is `[text | {"marker": refType}, seq, client, rseq, rclient, overlap, props]`: removed
when rclient != -1, its removal pending when rseq == -1 as well.
"""


def is_removed(seg):
    return seg[4] != -1


def local_length(seg):
    """nodeLength of a leaf in the editing client's local view (localNetLength)."""
    if is_removed(seg):
        return 0
    return 1 if isinstance(seg[0], dict) else len(seg[0].encode('utf-16-le', 'surrogatepass')) // 2


def break_tie(seg, own):
    """breakTie(0, 0, leaf, currentSeq, own): false only for a removal that has been sequenced."""
    return not (is_removed(seg) and seg[3] != -1)


def place(segs, own, ordinal, offset):
    """(split, leaf index of the new segment) for a reference on leaf `ordinal` at `offset` (its
    getOffset(): 0 on a removed segment) of the canonical leaves `segs` before the insert."""
    if not 0 <= ordinal < len(segs):
        raise IndexError('the reference names no linked leaf')
    split = offset != 0 and local_length(segs[ordinal]) != 0
    if split:
        return True, ordinal + 1  # the left half in front of the right one has local length: no excursion
    start = ordinal
    i = ordinal - 1
    while i >= 0 and local_length(segs[i]) == 0:
        if break_tie(segs[i], own):
            start = i
        i -= 1
    return False, start


def segs_of_flags(flags, own):
    """Canonical leaves, as far as `place` reads them, of one character per leaf: '.' live, 'x'
    removed and acked, 'p' removal pending (tests/golden/refinsert.expected.jsonl `pre`)."""
    return [['a', 1, 2, {'.': -1, 'x': 1, 'p': -1}[f], {'.': -1, 'x': 2, 'p': own}[f], [], None] for f in flags]


def lower(batch, doc, ats):
    """The records of document `doc` of an oplog.OpBatch whose type-5 records name reference ids, with
    each lowered to MT_OP_INSERT_AT at (ordinal, offset) of `ats` (one {op, refOrd, refOff} row per such
    record, in order; op None: a detached reference, the record is dropped).  A one-document OpBatch."""
    import numpy as np
    from .oplog import INSERT_AT, OpBatch, base_type
    one = batch.doc_slice(doc, doc + 1)
    ops = one.ops.copy()
    keep = np.ones(len(ops), dtype=bool)
    rows = iter(ats)
    for i, r in enumerate(ops):
        if r['seq'] == -1 and base_type(r['type']) == INSERT_AT:
            a = next(rows)
            if a['op'] is None:
                keep[i] = False
            else:
                ops[i]['pos1'], ops[i]['pos2'] = a['refOrd'], a['refOff']
    ops = ops[keep]
    return OpBatch(ops, one.payload, np.array([0, len(ops)], dtype=np.uint32))
