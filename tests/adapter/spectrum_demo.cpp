// Drives the sanity block of elliptic_interface.cc:973-1009 through include/alfd/dealii_adapter.hpp against the mock
// deal.II classes: solve as adapter_demo's `elliptic` mode does, then the constraint residual and the condition-number
// estimate of C Ct.  Prints "constraint_residual=<r> bound=<b>" and "kappa=<k> steps=<n> converged=<0|1>"; exit code 3
// if no GPU context can be created.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "alfd/dealii_adapter.hpp"
#include "mock_dealii.hpp"

#include "../../fictitious_domain_al_preconditioners_amd/csrc/synth/synth.h"

static mock::SparseMatrix load(void *h, const char *name) {
  int64_t m, n, nnz;
  const int64_t *rp;
  const int32_t *col;
  const double *val;
  if (alfd_synth_matrix(h, name, &m, &n, &nnz, &rp, &col, &val) != 0) throw std::runtime_error(name);
  return mock::SparseMatrix((size_t)m, (size_t)n, (const long *)rp, col, val);
}

static int run() {
  using namespace alfd::dealii_adapter;
  alfd_synth_params sp;
  std::memset(&sp, 0, sizeof(sp));
  sp.u_node0 = sp.u_node1 = sp.p_node0 = sp.p_node1 = sp.l0 = sp.l1 = -1;
  sp.beta = 1;
  sp.dim = 2, sp.degree = 1, sp.ncomp = 1, sp.n_cells = 32, sp.lo = -1, sp.hi = 1, sp.coupling_nq = 3;
  sp.body_force[0] = 1.0;
  sp.immersed_kind = 1, sp.imm_lo = -0.14, sp.imm_hi = 0.47, sp.imm_cells = 8, sp.beta2 = 10.0 - 1.0;
  char err[256];
  void *h = alfd_synth_generate(&sp, err, 256);
  if (!h) return std::fprintf(stderr, "generator: %s\n", err), 2;
  mock::SparseMatrix stiffness_matrix_bg = load(h, "A"), stiffness_matrix_fg = load(h, "A2"),
                     coupling_matrix = load(h, "Ct"), mass_matrix_fg = load(h, "M");
  const size_t n_bg = stiffness_matrix_bg.m(), n_fg = mass_matrix_fg.m();
  mock::Vector inverse_diag_mass_squared(n_fg);
  for (size_t i = 0; i < n_fg; ++i) {
    double d = 0;
    for (auto it = mass_matrix_fg.begin(i); it != mass_matrix_fg.end(i); ++it) d += it->value() * it->value();
    inverse_diag_mass_squared[i] = 1. / d;
  }
  System gpu(0);
  gpu.set_matrix(ALFD_A, stiffness_matrix_bg);
  gpu.set_matrix(ALFD_A2, stiffness_matrix_fg);
  gpu.set_matrix(ALFD_M, mass_matrix_fg);
  gpu.set_matrix(ALFD_CT, coupling_matrix);
  gpu.set_diag(ALFD_INVW, inverse_diag_mass_squared);
  alfd_config cfg;
  alfd_default_config(&cfg, ALFD_AL_ELL_MODIFIED);
  cfg.gamma = 10, cfg.gamma2 = 1e-2;
  cfg.inner = {ALFD_CTRL_REDUCTION, 100000, 1e-2, 1e-20};
  cfg.outer = {ALFD_CTRL_REDUCTION, 1000, 1e-10, 1e-10};
  gpu.configure(cfg);
  gpu.setup();
  mock::BlockVector system_solution_block({n_bg, n_fg, n_fg}), system_rhs_block({n_bg, n_fg, n_fg});
  int64_t n;
  const double *f, *f2;
  alfd_synth_vector(h, "f", &n, &f);
  for (size_t i = 0; i < n_bg; ++i) system_rhs_block.block(0)[i] = f[i];
  alfd_synth_vector(h, "f2", &n, &f2);
  for (size_t i = 0; i < n_fg; ++i) system_rhs_block.block(1)[i] = f2[i];
  double rhs_norm = 0;
  for (unsigned int b = 0; b < 3; ++b)
    for (size_t i = 0; i < system_rhs_block.block(b).size(); ++i) rhs_norm += system_rhs_block.block(b)[i] * system_rhs_block.block(b)[i];
  rhs_norm = std::sqrt(rhs_norm);
  auto system_operator = gpu.system_operator();
  EllipticInterfacePreconditioners::BlockTriangularALPreconditionerModified preconditioner_AL(gpu);
  SolverFGMRES<mock::BlockVector> solver_fgmres(gpu);
  solver_fgmres.solve(system_operator, system_solution_block, system_rhs_block, preconditioner_AL);
  // if (parameters.do_sanity_checks) { ... }   elliptic_interface.cc:973-1009
  const double residual = gpu.constraint_residual(system_solution_block, system_rhs_block.block(2));
  const double residual0 = gpu.constraint_residual(system_solution_block);   // the rhs row is zero: same number
  std::printf("constraint_residual=%.17g same=%d bound=%.17g\n", residual, residual == residual0 ? 1 : 0,
              std::max(cfg.outer.tol, cfg.outer.reduce * rhs_norm));
  const alfd_spectrum s = gpu.estimate_condition_number_CCt();
  std::printf("kappa=%.17g steps=%d converged=%d\n", s.condition, s.steps, s.converged);
  bool refused = false;   // a bad control goes through the status-to-exception mapping
  try {
    const alfd_control bad = {ALFD_CTRL_ABS, 0, 1e-12, 0.0};
    gpu.estimate_condition_number_CCt(&bad);
  } catch (const Error &e) {
    refused = e.status == ALFD_E_INVALID;
  }
  std::printf("refused=%d\n", refused ? 1 : 0);
  alfd_synth_free(h);
  return 0;
}

int main() {
  try {
    return run();
  } catch (const alfd::dealii_adapter::Error &e) {
    std::fprintf(stderr, "alfd error %d: %s\n", e.status, e.what());
    return e.status == ALFD_E_HIP ? 3 : 1;
  }
}
