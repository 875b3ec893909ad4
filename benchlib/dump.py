"""`bench.py --dump-outputs DIR`: what the timed path computed in its last step, written as .npy files so that two
builds of the project can be compared output for output on the same seeded inputs.

A felt is four little-endian 64-bit limbs on the device; in the files it is eight little-endian 32-bit words, each held
exactly in a float64, so the comparison is bit-exact."""
import os

from .common import HEIGHT


def felts_f64(t):
    """int64 [n, 4] felts (a torch tensor on any device) -> float64 numpy [n, 8], word 0 the least significant."""
    import numpy as np
    a = np.ascontiguousarray(t.detach().cpu().numpy().astype("<i8"))
    return a.view("<u4").reshape(a.shape[0], 8).astype(np.float64)


def tree_inner_nodes(levels, nb, t, height=HEIGHT):
    """The inner nodes of tree t of a level-major forest buffer of nb trees (sp_merkle_forest_dev's layout: level k holds
    nb * 2^(height-k) felts, tree t at offset t * 2^(height-k) within it) as float64 [2^height - 1, 8]: level 1 first,
    the root last."""
    import numpy as np
    parts, off = [], 0
    for k in range(height + 1):
        width = 1 << (height - k)
        if k > 0:
            parts.append(felts_f64(levels[off + t * width: off + (t + 1) * width]))
        off += nb * width
    return np.concatenate(parts)


def merkle_outputs(slot, world, height=HEIGHT):
    """The last step of the last call issued on `slot` (bench.py's stream slot: the forest buffer of `last_nb` trees and,
    with N > 1 ranks, the top forest of the combine): this rank's 2^height-leaf tree and the job root."""
    nb = slot["last_nb"]
    levels = slot["levels"][nb]
    nodes = tree_inner_nodes(levels, nb, nb - 1, height)
    if world > 1:  # top forest of nb trees over the world sub-roots: its last nb rows are the job roots
        root = felts_f64(slot["top"][nb * (2 * world - 1) - 1: nb * (2 * world - 1)])
    else:
        root = nodes[-1:]
    return {"merkle_last_tree_inner_nodes": nodes, "merkle_last_tree_root": root}


def write_outputs(directory, arrays):
    """DIR/<name>.npy for every array; returns the paths written."""
    import numpy as np
    os.makedirs(directory, exist_ok=True)
    paths = []
    for name, arr in arrays.items():
        p = os.path.join(directory, name + ".npy")
        np.save(p, arr)
        paths.append(p)
    return paths
