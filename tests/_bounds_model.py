"""Second model of bt_atlas_tile_bounds (include/bevy_terrain_amd.h): each cell's texel rectangle sliced directly, every level on its own,
with no composition of a coarser level from a finer one.

Cell (cx, cy) of level k, s_k = (T / g) << k, covers x in [cx*s_k, min((cx+1)*s_k, T-1)] and y likewise.  Its value is (min, max) over those
texels; with skip_zero texels equal to 0 are left out and a cell without texels is (0xFFFF, 0)."""
import numpy as np

EMPTY = (0xFFFF, 0)


def cells_per_layer(grid):
    return (4 * grid * grid - 1) // 3


def tile_bounds(layers, grid, skip_zero=False):
    """layers: (count, T, T) uint16 -> [level k: (count, n_k, n_k, 2) uint16], finest first"""
    layers = np.asarray(layers)
    if layers.ndim == 2:
        layers = layers[None]
    count, T = layers.shape[0], layers.shape[1]
    assert layers.shape[2] == T and grid >= 1 and grid & (grid - 1) == 0 and T % grid == 0
    s = T // grid
    data = layers.astype(np.int32)
    masked = np.where(data == 0, 1 << 16, data) if skip_zero else data  # a left-out texel is above every value for the minimum
    levels = []
    k = 0
    while grid >> k:
        n, sk = grid >> k, s << k
        out = np.empty((count, n, n, 2), dtype=np.uint16)
        for cy in range(n):
            y0, y1 = cy * sk, min((cy + 1) * sk, T - 1) + 1
            for cx in range(n):
                x0, x1 = cx * sk, min((cx + 1) * sk, T - 1) + 1
                mn = masked[:, y0:y1, x0:x1].min(axis=(1, 2))
                out[:, cy, cx, 0] = np.where(mn == 1 << 16, 0xFFFF, mn)
                out[:, cy, cx, 1] = data[:, y0:y1, x0:x1].max(axis=(1, 2))  # 0 is the identity of the maximum: left-out zeros change nothing
        levels.append(out)
        k += 1
    return levels


def compose(level):
    """the 2x2 composition of one level (count, n, n, 2) -> (count, n/2, n/2, 2): min of the minimums, max of the maximums"""
    c = level.reshape(level.shape[0], level.shape[1] // 2, 2, level.shape[2] // 2, 2, 2)
    return np.stack([c[..., 0].min(axis=(2, 4)), c[..., 1].max(axis=(2, 4))], axis=-1)
