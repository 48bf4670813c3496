/* synth.h -- C interface of libalfd_synth.so, the synthetic fictitious-domain operator
 * generator (input tooling: it stands in for the deal.II assembly the reference does in
 * immersed_laplace.cc:278-496, stokes_immersed_boundary.cc:410-820, elliptic_interface.cc:450-670;
 * no solver arithmetic).  Python binds it in problems.py, the C++ adapter demo includes this header. */
#ifndef ALFD_SYNTH_H
#define ALFD_SYNTH_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct alfd_synth_params {
  int32_t dim, degree, ncomp, n_cells;
  double lo, hi;
  int32_t stokes, grad_div;
  double gamma_grad_div, beta;
  double center[3];
  double radius;
  int32_t immersed_refine, coupling_nq;
  double body_force[3];
  double embedded_value[3];
  int64_t u_node0, u_node1, p_node0, p_node1, l0, l1;
  int32_t immersed_kind, imm_cells;
  double imm_lo, imm_hi, beta2;
  int32_t want_surface_mass;
  /* 0: rows written in closed form from Kronecker products of 1-D element matrices (default);
   * 1: CELL-WISE assembly as deal.II does it (stokes_immersed_boundary.cc:668-760): ONE cell matrix integrated
   *    numerically (Gauss quadrature, Jacobian from the vertex coordinates of a cell), every global entry the
   *    floating-point sum of its cells' contributions in the order a refinement tree visits the cells
   *    (Morton / z-order of the cell coordinates) -- mathematically equal entries then differ in their last bits
   *    wherever the visiting order of the cells around a node differs.  Block (0,0) only (scalar / Stokes). */
  int32_t assembly;
  int32_t elasticity, pad2_;
  double lame_lambda, lame_mu, lame2_lambda, lame2_mu;
  double box_lo[3], box_hi[3];
  int32_t box_cells[3];
  /* 1: the Stokes velocity block is the reference's 2 eps(u):eps(v) form (stokes...:712-730) instead of
   * grad u : grad v; Kronecker assembly only.  2 eps:eps = grad:grad + T, block (b,a) of T = block (a,b) of the
   * gamma_gd = 1 grad-div matrix.  The grad-div term, if on, is added after T. */
  int32_t sym_grad;
  /* 1: ONE layer of local refinement of the background mesh near the immersed body (what `Local refinements steps
   * near embedded domain = 1` of parameters_stokes_3d.prm asks for).  Every base cell whose closed box holds a node
   * of the immersed mesh (a node on a shared face counts for the lower cell) and each of its face neighbours is
   * replaced by its 2^dim children.  Unknowns sit on the lattice of spacing h / (2 degree): base cells use every
   * second lattice point, children every one; numbering is lexicographic over the lattice points that carry a node.
   * A node of a child that lies in the closure of an unrefined cell without being one of its nodes is HANGING: its
   * constraint (the unrefined cell's shape functions at that point) is applied while the cell contributions are
   * added, its own row stays as a lone diagonal with a zero right-hand side, like a Dirichlet row.  Needs
   * assembly = 1, a surface-immersed body (immersed_kind 0), no elasticity, no sym_grad, no row ranges.
   * Extra vectors: u_points / p_points (dim doubles per node), u_hanging / p_hanging (0 / 1 per node),
   * flagged_cells (0 / 1 per base cell, x fastest). */
  int32_t local_refine;
} alfd_synth_params;

/* NULL on failure (message in err). */
void *alfd_synth_generate(const alfd_synth_params *sp, char *err, int errlen);
void alfd_synth_free(void *h);
/* Renumbers the NODES of the background / velocity space of a generated (unpartitioned) problem: node new_to_old[k]
 * becomes node k, all components of a node stay together.  A is permuted symmetrically, Bt / Ct by rows, B / C by
 * columns (entries of a row re-sorted by the new column index), f with the rows.  What a caller's DoF renumbering
 * (Cuthill-McKee, stokes_immersed_boundary.cc:533-541) does to the operators.  0 on success. */
int alfd_synth_permute_nodes(void *h, const int64_t *new_to_old, int64_t n_nodes);
/* 0 and dims/pointers if the matrix / vector exists, else -1; pointers stay valid until alfd_synth_free. */
int alfd_synth_matrix(void *h, const char *name, int64_t *nrows, int64_t *ncols, int64_t *nnz,
                      const int64_t **row_ptr, const int32_t **col, const double **val);
int alfd_synth_vector(void *h, const char *name, int64_t *n, const double **data);
void alfd_synth_transpose(int64_t nrows, int64_t ncols, const int64_t *row_ptr, const int32_t *col,
                          const double *val, int64_t *t_row_ptr, int32_t *t_col, double *t_val);

#ifdef __cplusplus
}
#endif
#endif
