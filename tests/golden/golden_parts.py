"""Golden vectors as ``.npz`` files of at most 1 MiB each.

``save(path, **arrays)`` writes ``path`` (``x.npz``) as one compressed file when that fits; otherwise as
``x.p0.npz``, ``x.p1.npz``, ...: every array cut along its first axis into chunks stored under
``<key>__<j>``, the chunks packed into part files in order.  ``load(path)`` returns the arrays of either
form as ``{key: array}``, bit for bit what was saved."""
import glob
import os

import numpy as np

LIMIT = 1 << 20  # bytes per file
PART_RAW = 900 * 1024  # raw bytes packed into one part file (compression only shrinks it; zip overhead is small)


def _part_files(path):
    stem = path[:-len(".npz")]
    files = glob.glob(glob.escape(stem) + ".p*.npz")
    return sorted(files, key=lambda f: int(f[len(stem) + 2:-len(".npz")]))


def save(path, **arrays):
    assert path.endswith(".npz")
    for old in _part_files(path) + [path]:
        if os.path.exists(old):
            os.remove(old)
    np.savez_compressed(path, **arrays)
    if os.path.getsize(path) <= LIMIT:
        return [path]
    os.remove(path)
    parts, cur, room = [], {}, PART_RAW
    for key, a in arrays.items():
        a = np.asarray(a)
        rows = a.shape[0] if a.ndim else 1
        step = max(1, PART_RAW // max(1, a.nbytes // max(rows, 1))) if a.ndim else 1
        chunks = [a[i:i + step] for i in range(0, rows, step)] if a.ndim and rows else [a]
        for j, c in enumerate(chunks):
            if cur and c.nbytes > room:
                parts.append(cur)
                cur, room = {}, PART_RAW
            cur[f"{key}__{j}"] = c
            room -= c.nbytes
    parts.append(cur)
    out = []
    for i, p in enumerate(parts):
        f = f"{path[:-len('.npz')]}.p{i}.npz"
        np.savez_compressed(f, **p)
        assert os.path.getsize(f) <= LIMIT, (f, os.path.getsize(f))
        out.append(f)
    return out


def load(path):
    if os.path.exists(path):
        with np.load(path, allow_pickle=False) as z:
            return {k: z[k] for k in z.files}
    files = _part_files(path)
    if not files:
        raise FileNotFoundError(path)
    chunks = {}
    for f in files:
        with np.load(f, allow_pickle=False) as z:
            for name in z.files:
                key, j = name.rsplit("__", 1)
                chunks.setdefault(key, {})[int(j)] = z[name]
    return {k: (c[0] if len(c) == 1 else np.concatenate([c[j] for j in range(len(c))], axis=0))
            for k, c in chunks.items()}
