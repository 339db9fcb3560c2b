"""Document checkpoints on the host: check, describe, read and write the blobs of
MergeEngine.save_docs (include/mtgpu.h "document checkpoints"; the layout: csrc/mt_ckpt.h).

Nothing here needs a device: mt_checkpoint_check / mt_checkpoint_doc are host code of libmtgpu.so.
"""
import ctypes

import numpy as np

from .engine import CheckpointError, MtError, _check, _ptr, lib

# mt_ckpt_why
WHY = {0: 'ok', 1: 'truncated', 2: 'magic', 3: 'version', 4: 'directory', 5: 'digest', 6: 'size', 7: 'scalars',
       8: 'blocks', 9: 'text', 10: 'heap', 11: 'ids', 12: 'pending', 13: 'refs', 14: 'intervals'}
# mt_ckpt_doc
DOC_DTYPE = np.dtype([('nseg', '<u4'), ('text_units', '<u4'), ('class_bits', '<u4'), ('pending', '<u4'),
                      ('refs', '<u4'), ('intervals', '<u4'), ('err', '<i4'), ('pad', '<u4'), ('bytes', '<u8')])
assert DOC_DTYPE.itemsize == 40
CLASS_BITS = {'editing': 0x40000000, 'groups': 0x08000000, 'lds': 0x20000000, 'c64': 0x10000000, 'wide': 0x04000000}


def _blob(blob):
    return np.ascontiguousarray(np.frombuffer(blob, dtype=np.uint8) if isinstance(blob, (bytes, bytearray)) else blob,
                                dtype=np.uint8)


def check(blob):
    """The number of documents of a good blob; CheckpointError (.bad, .why) for any other."""
    b = _blob(blob)
    n, bad, why = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    rc = lib().mt_checkpoint_check(_ptr(b), len(b), ctypes.byref(n), ctypes.byref(bad), ctypes.byref(why))
    if rc:
        raise CheckpointError(f'checkpoint: {WHY.get(why.value, why.value)} (document {bad.value})', bad.value,
                              why.value)
    return n.value


def describe(blob):
    """The directory of a good blob: one dict per document."""
    b = _blob(blob)
    out = []
    for i in range(check(b)):
        d = np.zeros(1, dtype=DOC_DTYPE)
        _check(lib().mt_checkpoint_doc(_ptr(b), len(b), i, _ptr(d)), 'mt_checkpoint_doc')
        r = d[0]
        out.append({'nseg': int(r['nseg']), 'text_units': int(r['text_units']),
                    'classes': sorted(k for k, v in CLASS_BITS.items() if int(r['class_bits']) & v),
                    'pending': int(r['pending']), 'refs': int(r['refs']), 'intervals': int(r['intervals']),
                    'err': int(r['err']), 'bytes': int(r['bytes'])})
    return out


def write(path, blob):
    """The blob to a file, checked first (a bad blob is never written)."""
    b = _blob(blob)
    check(b)
    with open(path, 'wb') as fh:
        fh.write(b.tobytes())


def read(path):
    """A blob from a file, checked (CheckpointError for a damaged file)."""
    b = np.fromfile(path, dtype=np.uint8)
    check(b)
    return b


__all__ = ['check', 'describe', 'write', 'read', 'CheckpointError', 'MtError', 'WHY']
