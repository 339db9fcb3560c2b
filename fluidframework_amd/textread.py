"""Text reads of the batched engine (include/mtgpu.h "text reads").

`MergeTreeTextHelper.getText / getTextAndMarkers` (packages/dds/merge-tree/src/textSegment.ts:124-276)
walk `mapRange` -> `nodeMap` (mergeTree.ts:2903-2965) with `gatherText` as the leaf action; the engine
answers a batch of such reads on the device (`MergeEngine.text_ranges / text_lengths`).  This module
holds the record layouts of those calls and, in plain Python, the read itself over a canonical state
(`MergeEngine.state(doc)['segs']`: rows [text | {"marker": refType}, seq, client, removedSeq,
removedClient, overlap ids, props]).  Text is handled as UTF-16 code units throughout.
"""
import numpy as np

# mt_text_query / mt_text_marker / mt_text_count
TEXT_QUERY_DTYPE = np.dtype([('doc', '<u4'), ('start', '<i4'), ('end', '<i4'), ('ref_seq', '<i4'), ('client', '<u2'),
                             ('placeholder', '<u2'), ('flags', '<u4'), ('reserved', '<u4', (2,))])
TEXT_MARKER_DTYPE = np.dtype([('ordinal', '<i4'), ('out_offset', '<u4')])
TEXT_COUNT_DTYPE = np.dtype([('units', '<u4'), ('markers', '<u4')])
assert TEXT_QUERY_DTYPE.itemsize == 32 and TEXT_MARKER_DTYPE.itemsize == 8 and TEXT_COUNT_DTYPE.itemsize == 8

TEXT_MARKERS = 1             # mt_text_query.flags: list the visited markers
TEXT_BAD_QUERY = 0xFFFFFFFF  # mt_text_count.units of a query the device refused
TEXT_LOCAL = -2**31          # ref_seq of the local view (MT_POS_LOCAL)
TEXT_END = 2**31 - 1         # an `end` past every view


def units(text):
    """A str as its UTF-16 code units (lone surrogates kept)."""
    return np.frombuffer(text.encode('utf-16-le', 'surrogatepass'), dtype='<u2')


def from_units(u):
    return np.asarray(u, dtype='<u2').tobytes().decode('utf-16-le', 'surrogatepass')


def is_marker(seg):
    return isinstance(seg[0], dict)


def cached_length(seg):
    """cachedLength: UTF-16 code units (textSegment.ts:45); a marker is 1."""
    return 1 if is_marker(seg) else len(units(seg[0]))


def view_len(seg, ref_seq, client):
    """nodeLength's leaf branch (mergeTree.ts:1659-1697) over a canonical segment row; ref_seq None:
    the local view (pending inserts count, pending removals hide)."""
    seq, cl, rseq, rcl, ovl = seg[1], seg[2], seg[3], seg[4], seg[5]
    removed = rcl != -1 or rseq != -1
    if ref_seq is None:
        return 0 if removed else cached_length(seg)
    if not (cl == client or (seq != -1 and seq <= ref_seq)):
        return 0
    if removed and (rcl == client or client in ovl or (rseq != -1 and rseq <= ref_seq)):
        return 0
    return cached_length(seg)


def get_length(segs, ref_seq=None, client=0):
    """MergeTree.getLength(refSeq, clientId)."""
    return sum(view_len(s, ref_seq, client) for s in segs)


def get_text(segs, start=None, end=None, ref_seq=None, client=0, placeholder=''):
    """(text, markers): getText(refSeq, clientId, placeholder, start, end) over the leaves in order,
    and every visited marker as (ordinal, out_offset) with out_offset the units of `text` before it.
    `placeholder` is '' or one UTF-16 unit ('*' is composed by the caller: compose_star)."""
    if start is None:
        start = 0
    if end is None:
        end = get_length(segs, ref_seq, client)
    out, markers, n, p = [], [], 0, 0
    for i, s in enumerate(segs):
        ln = view_len(s, ref_seq, client)
        if ln > 0 and end - p > 0 and start - p < ln:  # nodeMap's test (mergeTree.ts:2937)
            if is_marker(s):
                markers.append((i, n))
                if placeholder:
                    out.append(units(placeholder))
                    n += 1
            else:
                a, b = min(max(start - p, 0), ln), min(max(end - p, 0), ln)
                piece = units(s[0])[min(a, b):max(a, b)]  # String.substring, its argument swap included
                out.append(piece)
                n += len(piece)
        p += ln
    return from_units(np.concatenate(out) if out else np.zeros(0, '<u2')), markers


def marker_string(ref_type, props=None):
    """Marker.toString (mergeTree.ts:723-787) from the marker's refType and its properties as the
    reference holds them (None: undefined; "referenceTileLabels" / "referenceRangeLabels" label lists
    and "markerId" among them)."""
    import json
    b = ''
    if ref_type & 1:
        b += 'Tile'
    if ref_type & 2:
        b += ('; ' if b else '') + 'RangeBegin'
    if ref_type & 4:
        b += ('; ' if b else '') + 'RangeEnd'
    props_defined = props is not None
    props = props or {}
    if props.get('markerId'):
        b += ' (%s) ' % props['markerId']
    # hasTileLabels / hasRangeLabels (mergeTree.ts:581-586): by the refType as well as the property
    tile = props.get('referenceTileLabels') if ref_type & 1 else None
    rng = props.get('referenceRangeLabels') if ref_type & 6 else None
    lb = ''
    if tile:
        lb += 'tile -- ' + '; '.join(tile)
    if rng:
        lb += (' ' if tile else '') + 'range %s -- ' % ('end' if ref_type & 4 else 'begin') + '; '.join(rng)
    pb = json.dumps(props, separators=(',', ':'), ensure_ascii=False) if props_defined else ''
    return 'M ' + b + ': ' + lb + ' ' + pb


def has_tile_label(ref_type, props, label):
    """Marker.hasTileLabel (mergeTree.ts:581-597): a Tile marker whose "referenceTileLabels" holds it."""
    return bool(ref_type & 1) and label in ((props or {}).get('referenceTileLabels') or [])


def compose_star(text, markers, strings):
    """getText with the "*" placeholder: "\\n" + marker.toString() spliced in at each marker of a read
    made without placeholder (`strings[k]`: markers[k]'s toString())."""
    u = units(text)
    out, at = [], 0
    for (_, off), s in zip(markers, strings):
        out += [u[at:off], units('\n' + s)]
        at = off
    out.append(u[at:])
    return from_units(np.concatenate(out))


def split_at_markers(text, markers, labelled):
    """getTextAndMarkers' parallel arrays from a read without placeholder: the text is cut at every
    marker k with labelled[k] (hasTileLabel(label)); the run after the last such marker is dropped,
    as the reference drops it.  Returns (parallelText, the markers' ordinals)."""
    u = units(text)
    texts, ords, at = [], [], 0
    for (o, off), lab in zip(markers, labelled):
        if lab:
            texts.append(from_units(u[at:off]))
            ords.append(o)
            at = off
    return texts, ords
