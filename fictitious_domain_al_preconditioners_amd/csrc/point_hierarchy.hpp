// Geometric multigrid transfers from support points: host code only (no device, no context), behind
// alfd_host_point_lattice, alfd_host_point_prolongator, alfd_host_grid_prolongator and
// alfd_build_geometric_from_points.  The rule is stated once, in include/alfd/alfd.h; every weight is formed from two
// integers by one division (and one subtraction), so the transfers are those of problems.tensor_prolongators,
// refined_prolongators and immersed_tensor_prolongators entry for entry, whatever the numbering of the points.
#pragma once

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <memory>
#include <thread>
#include <utility>
#include <vector>

namespace point_hierarchy {

constexpr int64_t kMaxRows = 2147483000LL;
constexpr int64_t kMaxCells = 1LL << 30;

// rows [begin, end) of one of at most 16 contiguous slices, one thread each
template <class F>
static void parallel_slices(int64_t n, F &&body) {
  const int T = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(16u, std::max(1u, std::thread::hardware_concurrency())),
                                                           (n + 65535) / 65536));
  if (T == 1) return body(0, (int64_t)0, n);
  std::vector<std::thread> th;
  for (int t = 0; t < T; ++t) th.emplace_back([&body, n, t, T]() { body(t, n * t / T, n * (t + 1) / T); });
  for (auto &x : th) x.join();
}

// a vector whose resize() leaves the new elements uninitialised: the slices that fill them touch their pages first
template <class T>
struct uninitialised : std::allocator<T> {
  template <class U>
  struct rebind {
    using other = uninitialised<U>;
  };
  template <class U, class... Args>
  void construct(U *p, Args &&...args) {
    if constexpr (sizeof...(Args) == 0) ::new ((void *)p) U;
    else ::new ((void *)p) U(std::forward<Args>(args)...);
  }
};
template <class T>
using raw_vector = std::vector<T, uninitialised<T>>;

struct Lattice {
  int dim = 0;
  int64_t m[3] = {0, 0, 0};           // cells per axis
  double lo[3] = {0, 0, 0}, delta[3] = {0, 0, 0};
  raw_vector<int32_t> idx;            // [n][dim] lattice index of every point
  raw_vector<int64_t> node;           // [n] id of the point's lattice node in [0, n_ids)
  std::vector<int32_t> count;         // [n_ids] points on the node
  int64_t n_ids = 0, occupied = 0;
  bool complete = false;
};

// the distinct coordinates of one axis, ascending
static void distinct_sorted(int64_t n, int dim, const double *points, int d, std::vector<double> &u) {
  u.clear();
  bool many = false;
  double last = std::nan("");
  for (int64_t i = 0; i < n && !many; ++i) {
    const double x = points[i * dim + d];
    if (x == last) continue;
    last = x;
    auto it = std::lower_bound(u.begin(), u.end(), x);
    if (it != u.end() && *it == x) continue;
    if (u.size() >= 4096) many = true;
    else u.insert(it, x);
  }
  if (!many) return;
  u.resize((size_t)n);
  for (int64_t i = 0; i < n; ++i) u[(size_t)i] = points[i * dim + d];
  std::sort(u.begin(), u.end());
  u.erase(std::unique(u.begin(), u.end()), u.end());
}

// false: the points are no lattice (or an argument is out of range)
static bool lattice(int64_t n, int dim, const double *points, Lattice &L) {
  if (n < 1 || n > kMaxRows || dim < 1 || dim > 3 || !points) return false;
  L = Lattice();
  L.dim = dim;
  std::atomic<bool> bad{false};
  parallel_slices(n * dim, [&](int, int64_t a, int64_t b) {
    bool f = true;
    for (int64_t i = a; i < b; ++i) f = f && std::isfinite(points[i]);
    if (!f) bad = true;
  });
  if (bad) return false;
  std::vector<double> u;
  for (int d = 0; d < dim; ++d) {
    distinct_sorted(n, dim, points, d, u);
    const double lo = u.front(), span = u.back() - lo, tol = 1e-9 * span;
    double delta = 0.0;
    for (size_t k = 0; k + 1 < u.size(); ++k) {
      const double g = u[k + 1] - u[k];
      if (g > tol && (delta == 0.0 || g < delta)) delta = g;
    }
    L.lo[d] = lo;
    L.delta[d] = delta;
    if (delta > 0.0) {
      const double cells = span / delta;
      if (!(cells < (double)kMaxCells)) return false;
      L.m[d] = std::llround(cells);
    }
  }
  L.idx.resize((size_t)n * dim);
  parallel_slices(n, [&](int, int64_t a, int64_t b) {
    bool on = true;
    for (int64_t i = a; i < b; ++i)
      for (int d = 0; d < dim; ++d) {
        const double x = points[i * dim + d] - L.lo[d], h = L.delta[d];
        const int64_t k = h > 0.0 ? (int64_t)(x / h + 0.5) : 0;   // x >= 0: round to nearest
        if (k < 0 || k > L.m[d] || std::fabs(x - (double)k * h) > 1e-6 * h) on = false;
        L.idx[(size_t)i * dim + d] = (int32_t)k;
      }
    if (!on) bad = true;
  });
  if (bad) return false;
  // lattice nodes: x fastest.  A lattice of at most 16 n nodes is indexed directly, a sparser one through its sorted keys.
  double nodes = 1.0;
  for (int d = 0; d < dim; ++d) nodes *= (double)(L.m[d] + 1);
  const bool dense = nodes <= 16.0 * (double)n + 65536.0;
  L.node.resize((size_t)n);
  auto key = [&](int64_t i) {
    int64_t k = 0;
    for (int d = dim - 1; d >= 0; --d) k = k * (L.m[d] + 1) + L.idx[(size_t)i * dim + d];
    return k;
  };
  if (dense) {
    L.n_ids = (int64_t)nodes;
    parallel_slices(n, [&](int, int64_t a, int64_t b) {
      for (int64_t i = a; i < b; ++i) L.node[(size_t)i] = key(i);
    });
  } else {
    if (nodes >= 9.0e18) return false;
    std::vector<std::pair<int64_t, int64_t>> ks((size_t)n);
    for (int64_t i = 0; i < n; ++i) ks[(size_t)i] = {key(i), i};
    std::sort(ks.begin(), ks.end());
    int64_t id = -1;
    for (int64_t a = 0; a < n; ++a) {
      if (a == 0 || ks[(size_t)a].first != ks[(size_t)a - 1].first) ++id;
      L.node[(size_t)ks[(size_t)a].second] = id;
    }
    L.n_ids = id + 1;
  }
  L.count.assign((size_t)L.n_ids, 0);
  for (int64_t i = 0; i < n; ++i) ++L.count[(size_t)L.node[(size_t)i]];
  for (int32_t c : L.count) L.occupied += c > 0;
  L.complete = (double)L.occupied == nodes;
  return true;
}

struct Csr {
  int64_t nrows = 0, ncols = 0;
  std::vector<int64_t> rp;
  raw_vector<int32_t> col;
  raw_vector<double> val;
};

// The rows of one transfer.  Row r sits at node idx[r * dim + d] of a grid of fine[d] cells, carries component
// comp[r] (NULL: r % ncomp) and is live unless dead[r] (NULL: all live); the coarse grid has coarse[d] cells and its
// unknowns are the interior nodes (all nodes with boundary_unknowns), x fastest, node-major.  Per axis
// num = i * coarse, j = num / fine, rem = num % fine: weight 1 on node j when rem == 0, else fr = (double)rem / (double)fine
// with 1.0 - fr on j and fr on j + 1; 0 < fr < 1 and 1.0 - fr >= 2^-53, so no weight and no product of three is zero.
static void transfer_rows(int64_t n, int dim, const int32_t *idx, const int32_t *comp, const uint8_t *dead, int ncomp,
                          const int64_t *fine, const int64_t *coarse, bool boundary_unknowns, Csr &P) {
  int64_t stride[3] = {1, 1, 1};
  for (int d = 0; d < dim; ++d) stride[d] = boundary_unknowns ? coarse[d] + 1 : coarse[d] - 1;
  P.nrows = n;
  P.ncols = stride[0] * stride[1] * stride[2] * ncomp;
  P.rp.resize((size_t)n + 1);
  P.rp[0] = 0;
  // per axis one table over the fine nodes: the coarse unknowns a node takes from and their weights
  struct Axis {
    int cnt;
    int32_t node[2];
    double w[2];
  };
  std::vector<Axis> tab[3];
  for (int d = 0; d < 3; ++d) {
    if (d >= dim) {
      tab[d].assign(1, Axis{1, {0, 0}, {1.0, 0.0}});
      continue;
    }
    tab[d].assign((size_t)fine[d] + 1, Axis{0, {0, 0}, {0.0, 0.0}});
    for (int64_t i = 0; i <= fine[d]; ++i) {
      if (!boundary_unknowns && (i == 0 || i == fine[d])) continue;   // rows on the boundary are empty
      const int64_t num = i * coarse[d], j = num / fine[d], rem = num % fine[d];
      const double fr = (double)rem / (double)fine[d];
      Axis &a = tab[d][(size_t)i];
      for (int s = 0; s < (rem == 0 ? 1 : 2); ++s) {
        const int64_t c = j + s, k = boundary_unknowns ? c : c - 1;      // the coarse node and its number along d
        if (k < 0 || k >= stride[d]) continue;                             // no unknown there
        a.node[a.cnt] = (int32_t)k;
        a.w[a.cnt++] = rem == 0 ? 1.0 : (s == 0 ? 1.0 - fr : fr);
      }
    }
  }
  auto axis = [&](int64_t r, int d) -> const Axis & { return d < dim ? tab[d][(size_t)idx[r * dim + d]] : tab[d][0]; };
  parallel_slices(n, [&](int, int64_t a, int64_t b) {
    for (int64_t r = a; r < b; ++r)
      P.rp[(size_t)r + 1] = dead && dead[r] ? 0 : (int64_t)axis(r, 0).cnt * axis(r, 1).cnt * axis(r, 2).cnt;
  });
  for (int64_t r = 0; r < n; ++r) P.rp[(size_t)r + 1] += P.rp[(size_t)r];
  P.col.resize((size_t)P.rp[(size_t)n]);
  P.val.resize((size_t)P.rp[(size_t)n]);
  parallel_slices(n, [&](int, int64_t a, int64_t b) {
    for (int64_t r = a; r < b; ++r) {
      int64_t o = P.rp[(size_t)r];
      if (P.rp[(size_t)r + 1] == o) continue;
      const Axis &ax = axis(r, 0), &ay = axis(r, 1), &az = axis(r, 2);
      const int64_t c = comp ? comp[r] : r % ncomp;
      for (int z = 0; z < az.cnt; ++z)
        for (int y = 0; y < ay.cnt; ++y)
          for (int x = 0; x < ax.cnt; ++x, ++o) {
            const int64_t node = ((int64_t)az.node[z] * stride[1] + ay.node[y]) * stride[0] + ax.node[x];
            P.col[(size_t)o] = (int32_t)(node * ncomp + c);
            P.val[(size_t)o] = az.w[z] * (ay.w[y] * ax.w[x]);
          }
    }
  });
}

// the coarse grid below a grid of cur[] cells, and whether the rule adds that level
static bool next_cells(int dim, const int64_t *cur, bool boundary_unknowns, int64_t *next) {
  bool ok = true;
  for (int d = 0; d < dim; ++d) {
    next[d] = (cur[d] + 1) / 2;
    ok = ok && (boundary_unknowns ? cur[d] >= 2 : next[d] >= 2);
  }
  return ok;
}

static double grid_unknowns(int dim, int ncomp, const int64_t *cells, bool boundary_unknowns) {
  double k = ncomp;   // exact far beyond the sizes grid_sizes_ok() admits
  for (int d = 0; d < dim; ++d) k *= (double)(boundary_unknowns ? cells[d] + 1 : cells[d] - 1);
  return k;
}

// false: a size is out of range
static bool grid_sizes_ok(int dim, int ncomp, const int64_t *fine, const int64_t *coarse, bool boundary_unknowns,
                          bool rows_are_grid = true) {
  if (dim < 1 || dim > 3 || ncomp < 1 || ncomp > 64) return false;
  double rows = ncomp, cols = ncomp;
  for (int d = 0; d < dim; ++d) {
    if (coarse[d] < (boundary_unknowns ? 1 : 2) || coarse[d] > fine[d] || fine[d] > kMaxCells) return false;
    rows *= (double)(fine[d] + 1);
    cols *= (double)(coarse[d] + 1);
  }
  return (!rows_are_grid || rows <= (double)kMaxRows) && cols <= (double)kMaxRows;
}

// one lower level: the unknowns of a grid of fine[] cells from those of a grid of coarse[] cells
static bool grid_prolongator(int dim, int ncomp, const int64_t *fine, const int64_t *coarse, bool boundary_unknowns, Csr &P) {
  if (!grid_sizes_ok(dim, ncomp, fine, coarse, boundary_unknowns)) return false;
  int64_t span[3] = {1, 1, 1}, nodes = 1;
  for (int d = 0; d < dim; ++d) nodes *= span[d] = boundary_unknowns ? fine[d] + 1 : fine[d] - 1;
  std::vector<int32_t> idx((size_t)(nodes * ncomp * dim));
  for (int64_t k = 0; k < nodes; ++k) {
    int64_t rest = k;
    for (int d = 0; d < dim; ++d) {
      const int32_t i = (int32_t)(rest % span[d]) + (boundary_unknowns ? 0 : 1);
      rest /= span[d];
      for (int c = 0; c < ncomp; ++c) idx[(size_t)((k * ncomp + c) * dim + d)] = i;
    }
  }
  transfer_rows(nodes * ncomp, dim, idx.data(), nullptr, nullptr, ncomp, fine, coarse, boundary_unknowns, P);
  return true;
}

// Components and level 0.  ncomp == 0: taken from the first point's node.  comp_out[n] receives the components.
// false: a node with another number of unknowns than ncomp, a component out of range or twice on a node, an incomplete
// lattice without base, base cells out of range.
static bool point_components(int64_t n, const Lattice &L, int &ncomp, const int32_t *component, std::vector<int32_t> &comp) {
  if (ncomp == 0) ncomp = L.count[(size_t)L.node[0]];
  if (ncomp < 1 || ncomp > 64) return false;
  for (int32_t c : L.count)
    if (c != 0 && c != ncomp) return false;
  comp.resize((size_t)n);
  if (component) {
    std::vector<uint64_t> seen((size_t)L.n_ids, 0);
    for (int64_t i = 0; i < n; ++i) {
      const int32_t c = component[i];
      if (c < 0 || c >= ncomp) return false;
      uint64_t &s = seen[(size_t)L.node[(size_t)i]];
      if (s >> c & 1) return false;
      s |= (uint64_t)1 << c;
      comp[(size_t)i] = c;
    }
  } else {   // the rank among the node's unknowns by ascending index
    std::vector<int32_t> next((size_t)L.n_ids, 0);
    for (int64_t i = 0; i < n; ++i) comp[(size_t)i] = next[(size_t)L.node[(size_t)i]]++;
  }
  return true;
}

// the base grid of level 0: given, or (m + 1) / 2 cells per axis.  false: out of range
static bool base_cells(int dim, const int64_t *m, const int32_t *base, bool boundary_unknowns, int64_t *cells) {
  for (int d = 0; d < dim; ++d) {
    cells[d] = base ? base[d] : (m[d] + 1) / 2;
    if (cells[d] < (boundary_unknowns ? 1 : 2) || cells[d] > m[d]) return false;
  }
  return true;
}

// The level rule, stated once: the coarse grid of every level ([levels][dim] in cells) for a lattice of m[] cells.
// Level 0 maps onto the base grid; while its n_coarse > min_coarse and fewer than max_levels levels exist, a level onto
// the halved grid follows, provided next_cells() allows it.  With boundary unknowns a lattice direction of fewer than two
// cells gives no level at all (true, cells empty).  false: the base grid is out of range.
static bool level_cells(int dim, int ncomp, const int64_t *m, const int32_t *base, bool boundary_unknowns, int64_t min_coarse,
                        int max_levels, std::vector<int64_t> &cells) {
  cells.clear();
  if (boundary_unknowns)
    for (int d = 0; d < dim; ++d)
      if (m[d] < 2) return true;
  int64_t cur[3] = {1, 1, 1}, next[3] = {1, 1, 1};
  if (!base_cells(dim, m, base, boundary_unknowns, cur)) return false;
  cells.insert(cells.end(), cur, cur + dim);
  int levels = 1;
  while (grid_unknowns(dim, ncomp, cur, boundary_unknowns) > (double)min_coarse && levels < max_levels &&
         next_cells(dim, cur, boundary_unknowns, next)) {
    std::copy(next, next + dim, cur);
    cells.insert(cells.end(), cur, cur + dim);
    ++levels;
  }
  return true;
}

static bool point_prolongator(int64_t n, const Lattice &L, int ncomp, const int32_t *component, const uint8_t *constrained,
                              const int32_t *base, bool boundary_unknowns, Csr &P, int64_t *cells) {
  std::vector<int32_t> comp;
  if (!base && !L.complete) return false;   // a lattice with holes has no base grid of its own
  if (!point_components(n, L, ncomp, component, comp) || !base_cells(L.dim, L.m, base, boundary_unknowns, cells)) return false;
  if (!grid_sizes_ok(L.dim, ncomp, L.m, cells, boundary_unknowns, false)) return false;
  transfer_rows(n, L.dim, L.idx.data(), comp.data(), constrained, ncomp, L.m, cells, boundary_unknowns, P);
  return true;
}

// The whole hierarchy: level 0 from the points, then the grid levels of level_cells().  cells: the lattice, then the
// coarse grid of every level ((levels + 1) * dim entries).
static bool hierarchy(int64_t n, const Lattice &L, int ncomp, const int32_t *component, const uint8_t *constrained,
                      const int32_t *base, bool boundary_unknowns, int64_t min_coarse, int max_levels,
                      std::vector<Csr> &levels, std::vector<int64_t> &cells) {
  levels.clear();
  cells.assign(L.m, L.m + L.dim);
  if (ncomp == 0) ncomp = L.count[(size_t)L.node[0]];
  std::vector<int64_t> plan;
  if (ncomp < 1 || ncomp > 64 || !level_cells(L.dim, ncomp, L.m, base, boundary_unknowns, min_coarse, max_levels, plan))
    return false;
  const int dim = L.dim, nlev = (int)plan.size() / dim;
  for (int l = 0; l < nlev; ++l) {
    levels.emplace_back();
    int64_t c0[3];
    const bool ok = l == 0 ? point_prolongator(n, L, ncomp, component, constrained, base, boundary_unknowns, levels.back(), c0)
                           : grid_prolongator(dim, ncomp, &plan[(size_t)(l - 1) * dim], &plan[(size_t)l * dim],
                                              boundary_unknowns, levels.back());
    if (!ok) return levels.clear(), false;
  }
  cells.insert(cells.end(), plan.begin(), plan.end());
  return true;
}

}   // namespace point_hierarchy
