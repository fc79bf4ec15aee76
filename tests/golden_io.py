"""Reading and writing the fixture files of tests/golden/, each kept under 1 MB.

A set of arrays too large for one file is stored as ``<name>.npz``, ``<name>.part2.npz``, ... (each written by
``np.savez_compressed``); ``load`` reads the parts back as one set, ``save`` writes them.  Test infrastructure
only.
"""
import glob
import io
import os

import numpy as np

PART_LIMIT = 1000 * 1000   # bytes per file, below the repository's 1 MiB limit for a committed file


class ArraySet(dict):
    """The arrays of one fixture by name, with NpzFile's ``files``."""

    @property
    def files(self):
        return list(self)


def parts(path):
    """``path`` and its continuation files, in order."""
    base = path[:-len(".npz")]
    more = glob.glob(base + ".part[0-9]*.npz")
    return [path, *sorted(more, key=lambda p: int(p[len(base) + len(".part"):-len(".npz")]))]


def load(path):
    out = ArraySet()
    for p in parts(path):
        with np.load(p) as z:
            for k in z.files:
                out[k] = z[k]
    return out


def _compressed_size(name, a):
    buf = io.BytesIO()
    np.savez_compressed(buf, **{name: a})
    return buf.getbuffer().nbytes


def save(path, **arrays):
    """``np.savez_compressed(path, **arrays)``, continued in ``<name>.partN.npz`` wherever one file would pass
    PART_LIMIT.  The arrays keep their order; continuation files of an earlier, longer set are removed."""
    groups, size = [{}], 0
    for name, a in arrays.items():
        s = _compressed_size(name, np.asanyarray(a))
        if groups[-1] and size + s > PART_LIMIT:
            groups.append({})
            size = 0
        groups[-1][name] = a
        size += s
    for old in parts(path)[1:]:
        os.remove(old)
    base = path[:-len(".npz")]
    for i, g in enumerate(groups):
        np.savez_compressed(path if i == 0 else f"{base}.part{i + 1}.npz", **g)
