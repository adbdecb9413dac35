// geometry.h -- where the warehouse's pickup points, delivery points and spawn cells are
// (core.py:170-199), written once for the gfx950 library (build_tables() packs the device tables
// from it; k_pack / k_unpack use the delivery functions) and the host engine (make_geo() fills its
// Geo from it).  Plain C++17, host and device; needs nothing included before it.
#pragma once

#if defined(__HIPCC__)
#define WH_GEO_FN __host__ __device__ inline
#else
#define WH_GEO_FN inline
#endif

namespace wh_geo {

struct Cell {
  int x, y;
};

// Pickup point j (core.py:171-175): for x in racks, for y in racks: (x-1, y-1), (x, y-1), (x-1, y), (x, y)
WH_GEO_FN Cell pickup_cell(const int* racks, int NR, int j) {
  const int r = j >> 2, q = j & 3;
  return Cell{racks[r / NR] - 1 + (q & 1), racks[r % NR] - 1 + (q >> 1)};
}

// Two pickup points on one cell: a rack covers the coordinates {r - 1, r} on both axes, so the
// points are distinct cells exactly when every two rack coordinates (a repeated one included) are
// at least 2 apart.  Neither engine runs such a config (WH_ENOTSUP).
WH_GEO_FN bool racks_overlap(const int* racks, int NR) {
  for (int i = 0; i < NR; ++i)
    for (int k = i + 1; k < NR; ++k)
      if (racks[i] - racks[k] < 2 && racks[k] - racks[i] < 2) return true;
  return false;
}

// (x, y) is a pickup cell when both coordinates lie on a rack
WH_GEO_FN bool on_rack(const int* racks, int NR, int c) {
  for (int i = 0; i < NR; ++i)
    if (c == racks[i] - 1 || c == racks[i]) return true;
  return false;
}
WH_GEO_FN bool is_pickup_cell(const int* racks, int NR, int x, int y) {
  return on_rack(racks, NR, x) && on_rack(racks, NR, y);
}

// Delivery point d (core.py:178-188): for v in 2..D-3: (v, 0), (0, v), (v, D-1), (D-1, v)
WH_GEO_FN Cell delivery_cell(int d, int D) {
  const int v = 2 + (d >> 2), side = d & 3;
  return Cell{(side & 1) ? (side == 3 ? D - 1 : 0) : v, (side & 1) ? v : (side == 2 ? D - 1 : 0)};
}
// ... and its inverse, for a delivery cell
WH_GEO_FN int delivery_index(int x, int y, int D) {
  if (y == 0) return 4 * (x - 2);
  if (x == 0) return 4 * (y - 2) + 1;
  if (y == D - 1) return 4 * (x - 2) + 2;
  return 4 * (y - 2) + 3;
}

// Spawn cells (core.py:191-199): interior, not a pickup cell, ascending (x, y).  emit(x, y) per
// cell; returns how many there are.
template <class Emit>
inline int spawn_cells(const int* racks, int NR, int D, Emit emit) {
  int nv = 0;
  for (int x = 1; x < D - 1; ++x)
    for (int y = 1; y < D - 1; ++y)
      if (!is_pickup_cell(racks, NR, x, y)) {
        emit(x, y);
        ++nv;
      }
  return nv;
}

}  // namespace wh_geo
