"""Helpers to read and write the committed golden fixtures (tests/golden/*.npz).

No committed file may exceed 1 MiB, so a fixture too large for one file is stored in several:
`<name>.npz` keeps the small arrays (and `kind`), and `<name>.partK.npz` hold the large ones cut
into flat pieces `<key>__<i>` (their shape in `<key>__shape`). `load` puts them together again bit
for bit; callers see one dict either way.
"""
import glob
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def names(kind=None):
    out = []
    for p in sorted(glob.glob(os.path.join(GOLDEN, "*.npz"))):
        if ".part" in os.path.basename(p):
            continue
        if kind is None or str(np.load(p)["kind"]) == kind:
            out.append(os.path.splitext(os.path.basename(p))[0])
    return out


PIECE_BYTES = 256 << 10   # arrays above this are cut into pieces of this size
PART_BYTES = 896 << 10    # raw bytes per part file (compression only shrinks it): below 1 MiB on disk


def save(name, out_dir=GOLDEN, **arrays):
    """np.savez_compressed, spread over `<name>.npz` + `<name>.partK.npz` when large (see above)."""
    arrays = {k: np.asarray(v) for k, v in arrays.items()}
    for old in glob.glob(os.path.join(out_dir, name + ".part*.npz")):
        os.remove(old)
    np.savez_compressed(os.path.join(out_dir, name + ".npz"), **arrays)
    if os.path.getsize(os.path.join(out_dir, name + ".npz")) <= 1 << 20:   # fits in one file: stored whole
        return
    main, pieces = {}, []
    for k, v in arrays.items():
        if v.nbytes <= PIECE_BYTES:
            main[k] = v
            continue
        main[k + "__shape"] = np.asarray(v.shape, dtype=np.int64)
        flat = np.ascontiguousarray(v).reshape(-1)
        step = PIECE_BYTES // v.itemsize
        pieces += [(f"{k}__{i}", flat[o:o + step]) for i, o in enumerate(range(0, flat.size, step))]
    np.savez_compressed(os.path.join(out_dir, name + ".npz"), **main)
    part, size, n = {}, 0, 0
    for k, v in pieces + [(None, None)]:
        if part and (k is None or size + v.nbytes > PART_BYTES):
            n += 1
            np.savez_compressed(os.path.join(out_dir, f"{name}.part{n}.npz"), **part)
            part, size = {}, 0
        if k is not None:
            part[k] = v
            size += v.nbytes


def load(name, out_dir=GOLDEN):
    d = dict(np.load(os.path.join(out_dir, name + ".npz")))
    for p in sorted(glob.glob(os.path.join(out_dir, name + ".part*.npz"))):
        d.update(np.load(p))
    for k in [k for k in d if k.endswith("__shape")]:
        key, shape = k[:-len("__shape")], tuple(d.pop(k))
        n = sum(1 for q in d if q.startswith(key + "__"))
        d[key] = np.concatenate([d.pop(f"{key}__{i}") for i in range(n)]).reshape(shape)
    return d


def bf16(u16):
    """uint16 bf16 bit patterns -> fp32 torch tensor (exact)."""
    a = np.asarray(u16).astype(np.uint32) << 16
    return torch.from_numpy(a.view(np.float32).copy())
