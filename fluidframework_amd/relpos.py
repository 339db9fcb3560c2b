"""Marker-relative positions on a canonical state: the rule of include/mtgpu.h ("marker-relative
positions"), restated in plain Python over the canonical JSON so that a log with
relative records can be lowered to an absolute one and the engine checked against both.

The reference: Client.getValidOpRange (client.ts:485-502) -> MergeTree.posFromRelativePos
(mergeTree.ts:1943-1966): marker = idToSegment[id]; without one the position is -1; else
getPosition(marker, refSeq, clientId) -- the view lengths of the leaves before it, whether or not the
view shows the marker -- plus 1 + offset, or minus offset for `before`.

A canonical segment is [text | {"marker": refType}, seq, client, rseq | -1, rclient | -1, [overlap],
props | None]; a pending local insert has seq -1, a pending local removal rseq -1 with its rclient.
"""
import numpy as np

from .oplog import ANNOTATE, INSERT, OP_REL, OpBatch, base_type, rel_len, split_payload

UNRESOLVED = -1


def is_marker(seg):
    return isinstance(seg[0], dict)


def seg_length(seg):
    """cachedLength: 1 for a Marker, else the text's UTF-16 code units."""
    return 1 if is_marker(seg) else len(seg[0].encode('utf-16-le', 'surrogatepass')) // 2


def removed(seg):
    return seg[4] != -1


def view_len(seg, ref_seq=None, client=None, own=None):
    """nodeLength's leaf branch (mergeTree.ts:1659-1697): the local view with ref_seq None, or for the
    editing client `own` itself; else what `client` had seen at ref_seq."""
    _, seq, c, rseq, rclient, ov, _ = seg
    if ref_seq is None or (own is not None and client == own):
        return 0 if removed(seg) else seg_length(seg)
    seen = c == client or (seq != -1 and seq <= ref_seq)
    hid = removed(seg) and (rclient == client or client in ov or (rseq != -1 and rseq <= ref_seq))
    return seg_length(seg) if seen and not hid else 0


def choose_marker(state, key, value):
    """Ordinal of the marker that value id `value` of key `key` names, None without one: among the
    linked Markers -- tombstones too -- whose current props hold it, the greatest insert seq (a pending
    insert above every sequenced one), the last in document order among equals.  Value id 0 names none."""
    if not value:
        return None
    best, rank = None, None
    for i, seg in enumerate(state['segs']):
        if not is_marker(seg) or seg[6] is None or seg[6].get('k%d' % key) != value:
            continue
        r = float('inf') if seg[1] == -1 else seg[1]
        if rank is None or r >= rank:
            best, rank = i, r
    return best


def marker_position(state, ordinal, ref_seq=None, client=None, own=None):
    """getPosition(segment, refSeq, clientId) (mergeTree.ts:1586-1603) of the leaf at `ordinal`."""
    return sum(view_len(s, ref_seq, client, own) for s in state['segs'][:ordinal])


def position_of(prefix, length, before, offset):
    """The relative position from the marker's: prefix - offset, or prefix + length + offset."""
    return prefix - offset if before else prefix + length + offset


def pos_from_relative(state, rel, ref_seq=None, client=None, own=None):
    """posFromRelativePos for rel = {key, value, before, offset}: UNRESOLVED (-1) without a marker."""
    k = choose_marker(state, rel['key'], rel['value'])
    if k is None:
        return UNRESOLVED
    return position_of(marker_position(state, k, ref_seq, client, own), seg_length(state['segs'][k]),
                       rel.get('before', False), rel.get('offset', 0))


def resolve(state, rec, payload, own=None):
    """(pos1, pos2, missing) of a record in `state`, the document's state before it: the absolute ends
    as they are, the relative ones in the record's view; missing counts the ends whose id names no
    marker (their position is UNRESOLVED)."""
    _, _, rel1, rel2 = split_payload(rec, payload)
    view = (int(rec['ref_seq']), int(rec['client']), own)
    p1, p2, missing = int(rec['pos1']), int(rec['pos2']), 0
    if rel1 is not None:
        p1 = pos_from_relative(state, rel1, *view)
        missing += choose_marker(state, rel1['key'], rel1['value']) is None
    if rel2 is not None:
        p2 = pos_from_relative(state, rel2, *view)
        missing += choose_marker(state, rel2['key'], rel2['value']) is None
    return p1, p2, missing


def lower(batch, states):
    """The batch with every relative record rewritten to the absolute record the rule gives.

    `states` is a replica that starts where the batch starts and follows it: `states.apply(OpBatch)`
    applies more records (of the already lowered log) and `states.state(doc)` reads a document's
    canonical state -- the CPU oracle, or an engine.  The log is lowered record by record: the replica
    is brought up to the relative record, the record is resolved in that state and substituted.

    A range whose ends are both unresolved -- the reference's (-1, -1), which touches nothing -- becomes
    the empty range (0, 0): no split, no segment, the callback without segments, zamboni and the window
    update, exactly as the engine applies it.  A record the engine refuses (an unresolved insert, a
    negative position, one unresolved end) keeps its negative position, which is refused likewise.
    The editing client's own sequenced relative record is the ack of an edit its host had resolved:
    only the blocks are cut off.  Returns (lowered OpBatch, [(doc, record index in the document, pos1,
    pos2, missing)] for every relative record a receiver resolves: the positions the rule gives, -1 for
    each of the `missing` ends whose id names no marker)."""
    ops = batch.ops.copy()
    payload = batch.payload
    resolved = []
    n = batch.n_docs

    def feed(d, lo, hi):
        if hi <= lo:
            return
        rp = np.zeros(n + 1, np.uint32)
        rp[d + 1:] = hi - lo
        states.apply(OpBatch(ops[lo:hi], payload, rp))

    for d in range(n):
        a, b = int(batch.row_ptr[d]), int(batch.row_ptr[d + 1])
        done, own = a, None
        for i in range(a, b):
            r = ops[i]
            if int(r['seq']) == -1 and own is None and base_type(r['type']) <= ANNOTATE:
                own = int(r['client'])
            if not int(r['type']) & OP_REL:
                continue
            typ = int(r['type'])
            if own is not None and int(r['client']) == own and int(r['seq']) >= 0:
                p1, p2 = int(r['pos1']), int(r['pos2'])   # the ack: positions play no part
            else:
                feed(d, done, i)
                done = i
                p1, p2, missing = resolve(states.state(d), r, payload, own)
                resolved.append((d, i - a, p1, p2, missing))
                if missing == 2 and base_type(typ) != INSERT:
                    p1 = p2 = 0
            ops[i]['pos1'], ops[i]['pos2'] = (max(min(p, 2**31 - 1), -2**31) for p in (p1, p2))
            ops[i]['payload_len'] = int(r['payload_len']) - rel_len(typ)
            ops[i]['type'] = typ & ~OP_REL
        feed(d, done, b)
    return OpBatch(ops, payload, batch.row_ptr), resolved
