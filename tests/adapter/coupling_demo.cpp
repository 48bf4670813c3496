// Drives System::update_coupling of include/alfd/dealii_adapter.hpp against the mock deal.II classes: the time loop of a
// fictitious-domain run whose circle moves over a fixed background mesh (immersed_laplace.cc's solve(), called once per
// position).  Position 0 is uploaded and set up in full; position 1 arrives through update_coupling and is solved from
// the previous solution; a second System that uploads position 1 from scratch solves from the same start.  Prints
//   "updated outer=<n> inner=<n> fresh outer=<n> inner=<n> same=<0|1>"   same: both solutions equal bit for bit
//   "products_a=<n> transfer_uploads=<n> power_iterations=<n>"            what the update ran
//   "refused=<0|1>"                                                        an update after a new A needs setup()
// Exit code 3 if no GPU context can be created.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

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

// problems.laplace2d_circle(32, 3) with the circle's centre at (cx, cy)
static void *generate(double cx, double cy) {
  alfd_synth_params sp;
  std::memset(&sp, 0, sizeof(sp));
  sp.u_node0 = sp.u_node1 = sp.p_node0 = sp.p_node1 = sp.l0 = sp.l1 = -1;
  sp.beta = 1;
  sp.dim = 2, sp.degree = 1, sp.ncomp = 1, sp.n_cells = 32, sp.lo = 0, sp.hi = 1;
  sp.center[0] = cx, sp.center[1] = cy, sp.radius = 0.2, sp.immersed_refine = 3, sp.coupling_nq = 3;
  sp.embedded_value[0] = 1.0;
  char err[256];
  void *h = alfd_synth_generate(&sp, err, 256);
  if (!h) throw std::runtime_error(err);
  return h;
}

static mock::Vector inverse_squares(const mock::SparseMatrix &mass_matrix) {   // immersed_laplace.cc:866-869
  mock::Vector d(mass_matrix.m());
  for (size_t i = 0; i < mass_matrix.m(); ++i) d[i] = 1. / (mass_matrix.diag_element(i) * mass_matrix.diag_element(i));
  return d;
}

static void rhs_of(void *h, alfd::dealii_adapter::System &sys, mock::BlockVector &rhs) {
  int64_t n;
  const double *g;
  alfd_synth_vector(h, "g", &n, &g);
  for (size_t i = 0; i < rhs.block(0).size(); ++i) rhs.block(0)[i] = 0;
  for (size_t i = 0; i < rhs.block(1).size(); ++i) rhs.block(1)[i] = g[i];
  sys.augment_rhs(rhs);
}

static int run() {
  using namespace alfd::dealii_adapter;
  void *h0 = generate(0.4, 0.4), *h1 = generate(0.43, 0.38);
  mock::SparseMatrix stiffness_matrix = load(h0, "A"), coupling0 = load(h0, "Ct"), mass0 = load(h0, "M"),
                     coupling1 = load(h1, "Ct"), mass1 = load(h1, "M");
  const size_t n_u = stiffness_matrix.m(), n_l = mass0.m();
  if (mass1.m() != n_l) return std::fprintf(stderr, "the two positions differ in size\n"), 2;
  alfd_config cfg;
  alfd_default_config(&cfg, ALFD_AL2);
  cfg.outer = {ALFD_CTRL_REDUCTION, 1000, 1e-10, 1e-12};
  cfg.inner.max_steps = 1000;

  System sys(0);
  sys.set_matrix(ALFD_A, stiffness_matrix);
  sys.set_matrix(ALFD_CT, coupling0);
  sys.set_diag(ALFD_INVW, inverse_squares(mass0));
  sys.configure(cfg);
  sys.setup();
  mock::BlockVector solution_block({n_u, n_l}), system_rhs_block({n_u, n_l});
  rhs_of(h0, sys, system_rhs_block);
  auto AA = sys.system_operator();
  BlockPreconditionerAugmentedLagrangian preconditioner(sys);
  SolverFGMRES<mock::BlockVector> solver_fgmres(sys);
  solver_fgmres.solve(AA, solution_block, system_rhs_block, preconditioner);
  mock::BlockVector start({n_u, n_l});
  for (unsigned int b = 0; b < 2; ++b)
    for (size_t i = 0; i < start.block(b).size(); ++i) start.block(b)[i] = solution_block.block(b)[i];

  // the body moved: only the coupling is new, the previous solution is the initial guess
  sys.update_coupling(coupling1, inverse_squares(mass1));
  const std::vector<int64_t> counts = sys.setup_counts();
  rhs_of(h1, sys, system_rhs_block);
  solver_fgmres.solve(AA, solution_block, system_rhs_block, preconditioner);
  const unsigned int outer_u = solver_fgmres.last_step();
  const long long inner_u = (long long)solver_fgmres.last_result().inner_iterations;

  // the same position uploaded from scratch
  System fresh(0);
  fresh.set_matrix(ALFD_A, stiffness_matrix);
  fresh.set_matrix(ALFD_CT, coupling1);
  fresh.set_diag(ALFD_INVW, inverse_squares(mass1));
  fresh.configure(cfg);
  fresh.setup();
  mock::BlockVector fresh_rhs({n_u, n_l});
  rhs_of(h1, fresh, fresh_rhs);
  auto AA_fresh = fresh.system_operator();
  BlockPreconditionerAugmentedLagrangian fresh_preconditioner(fresh);
  SolverFGMRES<mock::BlockVector> fresh_solver(fresh);
  fresh_solver.solve(AA_fresh, start, fresh_rhs, fresh_preconditioner);
  bool same = true;
  for (unsigned int b = 0; b < 2; ++b)
    for (size_t i = 0; i < start.block(b).size(); ++i) same = same && start.block(b)[i] == solution_block.block(b)[i];
  std::printf("updated outer=%u inner=%lld fresh outer=%u inner=%lld same=%d\n", outer_u, inner_u, fresh_solver.last_step(),
              (long long)fresh_solver.last_result().inner_iterations, same ? 1 : 0);
  std::printf("products_a=%lld transfer_uploads=%lld power_iterations=%lld\n", (long long)counts[ALFD_SC_PRODUCTS_A],
              (long long)counts[ALFD_SC_TRANSFER_UPLOADS], (long long)counts[ALFD_SC_POWER_ITERATIONS]);

  bool refused = false;   // a new A is not a coupling change: the status reaches the caller as an exception
  try {
    sys.set_matrix(ALFD_A, stiffness_matrix);
    sys.update_coupling(coupling0, inverse_squares(mass0));
  } catch (const Error &e) {
    refused = e.status == ALFD_E_INVALID && std::string(e.what()).find("alfd_setup") != std::string::npos;
  }
  sys.setup();            // which a full setup repairs
  std::printf("refused=%d\n", refused ? 1 : 0);
  alfd_synth_free(h0);
  alfd_synth_free(h1);
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
