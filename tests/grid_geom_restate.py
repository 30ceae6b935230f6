"""Scalar restatement of grid_map::GridMap::getSubmap, move, extendToInclude and addDataFrom (GM = grid_map_core/src/GridMap.cpp:
282-330, 442-507, 554-627, 514-552) and of what they call in GMM = GridMapMath.cpp, written from the reference text, as
include/liogpu.h lio_grid_submap, lio_grid_move, lio_grid_extend_to_include and lio_grid_add_data_from state them.  Python floats
are IEEE doubles and nothing here fuses a multiply with an add, so every operation is the fp64 operation the reference writes,
in its order; the loops are the reference's serial loops in GridMapIterator's order.  The map here is a real circular buffer
(startIndex), so that `move` clears rows and columns of the buffer as written and convertToDefaultStartIndex unwraps it through
getBufferRegionsForSubmap: the library's statement "new cell (r, c) takes old cell (r + shift0, c + shift1)" is derived from
that, not assumed.  Layers are held under integer ids, which stand for the reference's names.

What is not the reference's:
 - extendToInclude and addDataFrom ignore getIndex's verdict after isInside and would read past the buffer when it fails: such a
   cell is skipped and counted (n_index_outside);
 - submap_information(clamp=True), the library's form: a bounded corner whose getIndexFromPosition still fails is brought back
   to the last cell (lio_gm_bound_index), where the reference (clamp=False) returns false;
 - index_shift raises ValueError where the reference's cast is undefined (|v| >= 2^30 or not finite).
"""
import math

import numpy as np

import grid_sample_restate as gs
from grid_transform_restate import c_round

QNAN_BITS = 0x7fc00000
f32, u32 = np.float32, np.uint32
QNAN = np.array([QNAN_BITS], u32).view(f32)[0]
TOP_LEFT, TOP_RIGHT, BOTTOM_LEFT, BOTTOM_RIGHT, UNDEFINED = 0, 1, 2, 3, 4


def c_rem(a, n):
    """C's a % n: the quotient truncates toward zero"""
    return int(math.fmod(a, n))


def wrap_index(index, n):                                      # wrapIndexToRange, GMM:234-253
    if index < n:
        if index >= 0:
            return index
        if index >= -n:
            return index + n
        return c_rem(index, n) + n
    if index < n * 2:
        return index - n
    return c_rem(index, n)


def index_from_buffer_index(bi, size, start):                  # GMM:518-527
    if start == (0, 0):
        return tuple(bi)
    return tuple(wrap_index(bi[a] - start[a], size[a]) for a in range(2))


def buffer_index_from_index(index, size, start):               # GMM:529-538
    if start == (0, 0):
        return tuple(index)
    return tuple(wrap_index(index[a] + start[a], size[a]) for a in range(2))


def position_from_index(g, index, start=(0, 0)):               # getPositionFromIndex, GMM:130-145 (None: false)
    if not gs.in_range(index, g.size):
        return None
    u = index_from_buffer_index(index, g.size, start)
    return tuple(g.pos[a] + (0.5 * g.length[a] - 0.5 * g.res) + g.res * float(-u[a]) for a in range(2))


def index_from_position(g, p, start=(0, 0)):                   # getIndexFromPosition, GMM:147-160 -> (verdict, buffer index)
    index = tuple(gs._trunc(-((p[a] - 0.5 * g.length[a] - g.pos[a]) / g.res)) for a in range(2))
    index = buffer_index_from_index(index, g.size, start)
    return gs.within_map(g, p) and gs.in_range(index, g.size), index


def bound_position(g, p):                                      # boundPositionToRange, GMM:255-280
    out = []
    for a in range(2):
        shifted = p[a] - g.pos[a] + 0.5 * g.length[a]
        eps = 10.0 * np.finfo(np.float64).eps
        if math.fabs(p[a]) > 1.0:
            eps *= math.fabs(p[a])
        if shifted <= 0:
            shifted = eps
        elif shifted >= g.length[a]:
            shifted = g.length[a] - eps
        out.append(shifted + g.pos[a] - 0.5 * g.length[a])
    return tuple(out)


def half_transform(v):
    """halfTransform * v, halfTransform = 0.5 * getMapFrameToBufferOrderTransformation() = [[-0.5, -0], [-0, -0.5]]"""
    return (-0.5 * v[0] + -0.0 * v[1], -0.0 * v[0] + -0.5 * v[1])


def submap_information(g, requested_position, requested_length, start=(0, 0), clamp=False):
    """getSubmapInformation, GMM:287-341 -> None (false), or a dict: top_left (the buffer index), size, position, length,
    requested (the requested position's index in the submap)"""
    ht = half_transform(requested_length)
    corners = []
    for p in (tuple(requested_position[a] - ht[a] for a in range(2)), tuple(requested_position[a] + ht[a] for a in range(2))):
        verdict, index = index_from_position(g, bound_position(g, p), start)
        if not verdict:
            if not clamp:
                return None
            assert start == (0, 0)
            index = tuple(gs.clamp(index[a], g.size[a]) for a in range(2))
        corners.append(index)
    top_left_buffer = corners[0]
    top_left = index_from_buffer_index(corners[0], g.size, start)
    bottom_right = index_from_buffer_index(corners[1], g.size, start)
    corner = position_from_index(g, top_left_buffer, start)
    if corner is None:
        return None
    hr = half_transform((g.res, g.res))
    corner = tuple(corner[a] - hr[a] for a in range(2))
    size = tuple(bottom_right[a] - top_left[a] + 1 for a in range(2))
    length = tuple(float(size[a]) * g.res for a in range(2))
    position = tuple(corner[a] - 0.5 * length[a] for a in range(2))
    if size[0] < 1 or size[1] < 1:                             # (no index is in range of such a size)
        return None
    sub = gs.Geometry(size[0], size[1], g.res, position)
    assert sub.length == length
    verdict, requested = index_from_position(sub, requested_position)
    if not verdict:
        return None
    return dict(top_left=top_left_buffer, size=size, position=position, length=length, requested=requested)


def index_shift(position_shift, res):                          # getIndexShiftFromPositionShift, GMM:183-196, one component
    v = position_shift / res
    if not (math.fabs(v) < 2.0 ** 30):
        raise ValueError("the cast is undefined")
    return -int(v + 0.5 * (1 if v > 0 else -1))


def position_shift(shift, res):                                # getPositionShiftFromIndexShift, GMM:198-204
    return float(-shift) * res


def quadrant(index, start):                                    # getQuadrant, GMM:101-115
    if index[0] >= start[0] and index[1] >= start[1]:
        return TOP_LEFT
    if index[0] >= start[0] and index[1] < start[1]:
        return TOP_RIGHT
    if index[0] < start[0] and index[1] >= start[1]:
        return BOTTOM_LEFT
    return BOTTOM_RIGHT


def buffer_regions_for_submap(submap_index, submap_size, size, start):
    """getBufferRegionsForSubmap, GMM:351-459 -> None (false) or [(start index, size, quadrant)]"""
    u = index_from_buffer_index(submap_index, size, start)
    if u[0] + submap_size[0] > size[0] or u[1] + submap_size[1] > size[1]:
        return None
    si, ss = submap_index, submap_size
    br = tuple(wrap_index(si[a] + ss[a] - 1, size[a]) for a in range(2))
    q_tl, q_br = quadrant(si, start), quadrant(br, start)
    if q_tl == TOP_LEFT:
        if q_br == TOP_LEFT:
            return [(si, ss, TOP_LEFT)]
        if q_br == TOP_RIGHT:
            tl = (ss[0], size[1] - si[1])
            return [(si, tl, TOP_LEFT), ((si[0], 0), (ss[0], ss[1] - tl[1]), TOP_RIGHT)]
        if q_br == BOTTOM_LEFT:
            tl = (size[0] - si[0], ss[1])
            return [(si, tl, TOP_LEFT), ((0, si[1]), (ss[0] - tl[0], ss[1]), BOTTOM_LEFT)]
        tl = (size[0] - si[0], size[1] - si[1])
        tr = (size[0] - si[0], ss[1] - tl[1])
        bl = (ss[0] - tl[0], size[1] - si[1])
        return [(si, tl, TOP_LEFT), ((si[0], 0), tr, TOP_RIGHT), ((0, si[1]), bl, BOTTOM_LEFT), ((0, 0), (bl[0], tr[1]), BOTTOM_RIGHT)]
    if q_tl == TOP_RIGHT:
        if q_br == TOP_RIGHT:
            return [(si, ss, TOP_RIGHT)]
        if q_br == BOTTOM_RIGHT:
            tr = (size[0] - si[0], ss[1])
            return [(si, tr, TOP_RIGHT), ((0, si[1]), (ss[0] - tr[0], ss[1]), BOTTOM_RIGHT)]
    elif q_tl == BOTTOM_LEFT:
        if q_br == BOTTOM_LEFT:
            return [(si, ss, BOTTOM_LEFT)]
        if q_br == BOTTOM_RIGHT:
            bl = (ss[0], size[1] - si[1])
            return [(si, bl, BOTTOM_LEFT), ((si[0], 0), (ss[0], ss[1] - bl[1]), BOTTOM_RIGHT)]
    elif q_tl == BOTTOM_RIGHT:
        if q_br == BOTTOM_RIGHT:
            return [(si, ss, BOTTOM_RIGHT)]
    return None


def copy_regions(dst, src, regions):
    """the four corner assignments of GM:311-326 and GM:689-701: dst's corner of the region's size = src's block"""
    rows, cols = dst.shape
    for index, size, q in regions:
        block = src[index[0]:index[0] + size[0], index[1]:index[1] + size[1]]
        r0 = 0 if q in (TOP_LEFT, TOP_RIGHT) else rows - size[0]
        c0 = 0 if q in (TOP_LEFT, BOTTOM_LEFT) else cols - size[1]
        dst[r0:r0 + size[0], c0:c0 + size[1]] = block


def is_finite(v):
    return bool(np.isfinite(v))


class GridMap:
    """the members the four calls read and write; layers: {id: [rows, cols] float32 in buffer order}"""

    def __init__(self, ids=()):
        self.ids, self.data, self.basic = list(ids), {}, []
        self.size, self.res, self.length, self.pos, self.start = (0, 0), 0.0, (0.0, 0.0), (0.0, 0.0), (0, 0)

    @classmethod
    def of(cls, g, layers, basic=()):
        """a map of geometry g (gs.Geometry) holding `layers` ({id: array}, or a sequence: ids 0 ..)"""
        if not isinstance(layers, dict):
            layers = dict(enumerate(layers))
        m = cls(layers)
        m.size, m.res, m.length, m.pos = g.size, g.res, g.length, g.pos
        m.data = {k: np.array(v, f32).reshape(g.size).copy() for k, v in layers.items()}
        m.basic = list(basic)
        return m

    def copy(self):
        m = GridMap(self.ids)
        m.size, m.res, m.length, m.pos, m.start, m.basic = self.size, self.res, self.length, self.pos, self.start, list(self.basic)
        m.data = {k: v.copy() for k, v in self.data.items()}
        return m

    def set_geometry(self, length, res, pos):                  # GM:44-59
        self.size = (int(c_round(length[0] / res)), int(c_round(length[1] / res)))
        for k in self.ids:                                     # resize, clearAll
            self.data[k] = np.full(self.size, QNAN, f32)
        self.res = float(res)
        self.length = (float(self.size[0]) * self.res, float(self.size[1]) * self.res)
        self.pos = (float(pos[0]), float(pos[1]))
        self.start = (0, 0)

    def add(self, k, value=QNAN):                              # GM:82-98
        self.data[k] = np.full(self.size, value, f32)
        if k not in self.ids:
            self.ids.append(k)

    def words(self, ids=None):
        return np.stack([self.data[k].view(u32) for k in (self.ids if ids is None else ids)])

    def is_valid(self, index, layers=None):                    # GM:244-258
        layers = self.basic if layers is None else layers
        if not layers:
            return False
        return all(is_finite(self.data[k][index]) for k in layers)

    def cells(self):
        """GridMapIterator: the linear index ascending, column-major -> buffer indices"""
        rows, cols = self.size
        for lin in range(rows * cols):
            yield (lin % rows, lin // rows)

    # ---- move, GM:442-507
    def move(self, position):
        """-> (moved, the new regions [(start index, size)], the index shift)"""
        shift = tuple(index_shift(position[a] - self.pos[a], self.res) for a in range(2))
        aligned = tuple(position_shift(shift[a], self.res) for a in range(2))
        regions = []

        def clear(axis, index, n):                             # clearRows / clearCols: every layer
            for k in self.ids:
                if axis == 0:
                    self.data[k][index:index + n, :] = QNAN
                else:
                    self.data[k][:, index:index + n] = QNAN
            regions.append(((index, 0), (n, self.size[1])) if axis == 0 else ((0, index), (self.size[0], n)))

        for i in range(2):
            if shift[i] == 0:
                continue
            if abs(shift[i]) >= self.size[i]:
                for k in self.ids:
                    self.data[k][:, :] = QNAN
                regions.append(((0, 0), self.size))
                continue
            sign = 1 if shift[i] > 0 else -1
            start_index = self.start[i] - (1 if sign < 0 else 0)
            end_index = start_index - sign + shift[i]
            n_cells = abs(shift[i])
            index = wrap_index(start_index if sign > 0 else end_index, self.size[i])
            if index + n_cells <= self.size[i]:
                clear(i, index, n_cells)
            else:
                first = self.size[i] - index
                clear(i, index, first)
                clear(i, 0, n_cells - first)
        self.start = tuple(wrap_index(self.start[a] + shift[a], self.size[a]) for a in range(2))
        self.pos = tuple(self.pos[a] + aligned[a] for a in range(2))
        return shift != (0, 0), regions, shift

    def convert_to_default_start_index(self):                  # GM:677-707
        if self.start == (0, 0):
            return
        regions = buffer_regions_for_submap(self.start, self.size, self.size, self.start)
        assert regions is not None
        for k in self.ids:
            temp = self.data[k].copy()
            copy_regions(temp, self.data[k], regions)
            self.data[k] = temp
        self.start = (0, 0)

    # ---- getSubmap, GM:282-330
    def get_submap(self, position, length, clamp=False):
        """-> (the submap or None, submap_information's dict or None)"""
        info = submap_information(self, position, length, self.start, clamp)
        if info is None:
            return None, None
        sub = GridMap(self.ids)
        sub.basic = list(self.basic)
        sub.set_geometry(info["length"], self.res, info["position"])
        assert sub.size == info["size"]
        regions = buffer_regions_for_submap(info["top_left"], sub.size, self.size, self.start)
        if regions is None:
            return None, None
        for k in self.ids:
            copy_regions(sub.data[k], self.data[k], regions)
        return sub, info

    # ---- extendToInclude, GM:554-627
    def extend_to_include(self, other):
        """-> dict(resized, n_cells_kept, n_index_outside)"""
        top_left = [self.pos[a] + self.length[a] / 2.0 for a in range(2)]
        bottom_right = [self.pos[a] - self.length[a] / 2.0 for a in range(2)]
        top_left_other = [other.pos[a] + other.length[a] / 2.0 for a in range(2)]
        bottom_right_other = [other.pos[a] - other.length[a] / 2.0 for a in range(2)]
        resize, position, length = False, list(self.pos), list(self.length)
        for a in range(2):
            if top_left_other[a] > top_left[a]:
                position[a] += (top_left_other[a] - top_left[a]) / 2.0
                length[a] += top_left_other[a] - top_left[a]
                resize = True
        for a in range(2):
            if bottom_right_other[a] < bottom_right[a]:
                position[a] -= (bottom_right[a] - bottom_right_other[a]) / 2.0
                length[a] += bottom_right[a] - bottom_right_other[a]
                resize = True
        out = dict(resized=int(resize), n_cells_kept=0, n_index_outside=0)
        if not resize:
            return out
        old = self.copy()
        self.set_geometry(length, self.res, position)
        pos = list(self.pos)
        for a in range(2):
            shift = math.fmod(pos[a] - old.pos[a], self.res)
            if math.fabs(shift) < self.res / 2.0:
                pos[a] -= shift
            else:
                pos[a] += self.res - shift
            if self.size[a] % 2 != old.size[a] % 2:
                pos[a] += -math.copysign(self.res / 2.0, shift)
        self.pos = tuple(pos)
        for index in self.cells():
            if self.is_valid(index):
                continue
            p = position_from_index(self, index, self.start)
            if not gs.within_map(old, p):
                continue
            verdict, at = index_from_position(old, p, old.start)
            if not verdict:                                    # the labelled deviation
                out["n_index_outside"] += 1
                continue
            for k in self.ids:
                self.data[k].view(u32)[index] = old.data[k].view(u32)[at]
            out["n_cells_kept"] += 1
        return out

    # ---- addDataFrom, GM:514-552
    def add_data_from(self, other, extend, overwrite, copy_all, layers=()):
        """-> dict(resized, n_cells_skipped_valid, n_cells_outside_other, n_index_outside, n_values_copied)"""
        layers = list(other.ids) if copy_all else list(layers)
        ext = self.extend_to_include(other) if extend else dict(resized=0, n_index_outside=0)
        for k in layers:
            if k not in self.ids:
                self.add(k)
        out = dict(resized=ext["resized"], n_cells_skipped_valid=0, n_cells_outside_other=0, n_index_outside=ext["n_index_outside"], n_values_copied=0)
        for index in self.cells():
            if self.is_valid(index) and not overwrite:
                out["n_cells_skipped_valid"] += 1
                continue
            p = position_from_index(self, index, self.start)
            if not gs.within_map(other, p):
                out["n_cells_outside_other"] += 1
                continue
            verdict, at = index_from_position(other, p, other.start)
            if not verdict:                                    # the labelled deviation
                out["n_index_outside"] += 1
                continue
            for k in layers:
                if not is_finite(other.data[k][at]):
                    continue
                self.data[k].view(u32)[index] = other.data[k].view(u32)[at]
                out["n_values_copied"] += 1
        return out


# ---- the library's statements of the two calls that leave a start index or a fresh object in the reference
def lib_move(m, position):
    """move, then convertToDefaultStartIndex -> dict(moved, index_shift, position, n_cells_cleared); the cleared cells are
    counted on a layer of zeros that rides along"""
    m.add("mark", 0.0)
    moved, _, shift = m.move(position)
    m.convert_to_default_start_index()
    cleared = int(np.isnan(m.data["mark"]).sum())
    del m.data["mark"]
    m.ids.remove("mark")
    return dict(moved=int(moved), index_shift=shift, position=m.pos, n_cells_cleared=cleared)


def shifted_copy(layer, shift):
    """new cell (r, c) takes old cell (r + shift0, c + shift1) where that exists, the quiet NaN elsewhere"""
    rows, cols = layer.shape
    out = np.full((rows, cols), QNAN, f32)
    for r in range(rows):
        for c in range(cols):
            sr, sc = r + shift[0], c + shift[1]
            if 0 <= sr < rows and 0 <= sc < cols:
                out.view(u32)[r, c] = layer.view(u32)[sr, sc]
    return out
