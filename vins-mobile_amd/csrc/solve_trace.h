// solve_trace.h — what the three trust-region kernels (solver_core.h::minimize, pnp_core.h::solve, posegraph_kernel of
// vio_posegraph.hip) share of Ceres' TrustRegionMinimizer: the layout of the iteration trace a solve leaves in global
// memory with its writer and its host reader, the step evaluator and the traditional dogleg combination.
// Plain C++ for device and host code; nothing here synchronizes or knows about work-items.
#pragma once
#include <math.h>
#include <string.h>

#include "vio_amd.h"
#include "vio_math.h"

namespace vio {

// stats_d = [initial, final, -, -, it_cost[64], it_radius[64], it_step_norm[64], it_relative_decrease[64],
//            it_gradient_max_norm[64]]; stats_i = [iterations, termination, n_ok, n_bad, it_flags[64]]
constexpr int kMaxTrace = 64;
constexpr int kStatsDoubles = 4 + 5 * kMaxTrace;
constexpr int kStatsInts = 4 + kMaxTrace;
static_assert(kMaxTrace == VIO_MAX_TRACE, "the device trace and VioSolveStats hold the same number of iterations");

// Writer of one solve's trace. Every work-item may hold one; work-item 0 alone calls it.
struct SolveTrace {
  double *sd;
  int *si;
  VIO_HD void initial(double cost) const { sd[0] = cost; }
  // iteration record i (IterationSummary); records past the trace's capacity are dropped
  VIO_HD void record(int i, double cost, double radius, double step_norm, double rel, double gmax, bool valid, bool ok) const {
    if (i < kMaxTrace) {
      sd[4 + i] = cost, sd[4 + kMaxTrace + i] = radius, sd[4 + 2 * kMaxTrace + i] = step_norm;
      sd[4 + 3 * kMaxTrace + i] = rel, sd[4 + 4 * kMaxTrace + i] = gmax;
      si[4 + i] = (valid ? 1 : 0) | (ok ? 2 : 0);
    }
  }
  VIO_HD void finish(int recorded, int termination, int n_ok, int n_bad, double min_cost) const {
    sd[1] = min_cost;
    si[0] = recorded, si[1] = termination, si[2] = n_ok, si[3] = n_bad;
  }
};

// Host side: one solve's trace as the ABI's VioSolveStats. Trace slots at and past `iterations` are 0, whatever the raw
// arrays hold there (the kernels write the records they make and nothing else).
inline void unpack_solve_stats(const double *sd, const int *si, VioSolveStats *out) {
  memset(out, 0, sizeof(*out));
  out->initial_cost = sd[0], out->final_cost = sd[1];
  out->iterations = si[0], out->termination = si[1], out->num_successful_steps = si[2], out->num_unsuccessful_steps = si[3];
  for (int i = 0; i < si[0] && i < kMaxTrace; i++) {
    out->it_cost[i] = sd[4 + i], out->it_radius[i] = sd[4 + kMaxTrace + i], out->it_step_norm[i] = sd[4 + 2 * kMaxTrace + i];
    out->it_relative_decrease[i] = sd[4 + 3 * kMaxTrace + i], out->it_gradient_max_norm[i] = sd[4 + 4 * kMaxTrace + i];
    out->it_flags[i] = si[4 + i];
  }
}

// TrustRegionStepEvaluator (CSI/trust_region_step_evaluator.cc:38-107) without non-monotonic steps: every accepted step
// of a solve is a new minimum, and the reference follows the candidate at each.
// Passed and returned BY VALUE, members in this order: a member function takes the object's address, which keeps the six
// values in memory until the call is inlined, and either that or another member order changes the order in which the
// compiler turns them into registers -- enough to move the window kernel's register allocation (csrc/Makefile, WK_OPT).
struct StepEvaluator {
  double accumulated_candidate_model_cost_change, accumulated_reference_model_cost_change, candidate_cost, reference_cost,
      current_cost, minimum_cost;
  VIO_HD static StepEvaluator at(double initial_cost) { return {0, 0, initial_cost, initial_cost, initial_cost, initial_cost}; }
};
// StepQuality: rho of a step to a point of cost `cost`
VIO_HD double step_quality(StepEvaluator e, double cost, double model_cost_change) {
  const double rel = (e.current_cost - cost) / model_cost_change;
  const double hist = (e.reference_cost - cost) / (e.accumulated_reference_model_cost_change + model_cost_change);
  return fmax(rel, hist);
}
// StepAccepted
VIO_HD StepEvaluator step_accepted(StepEvaluator e, double cost, double model_cost_change) {
  e.current_cost = cost, e.accumulated_candidate_model_cost_change += model_cost_change;
  e.accumulated_reference_model_cost_change += model_cost_change;
  if (e.current_cost < e.minimum_cost) e.minimum_cost = e.current_cost, e.candidate_cost = e.current_cost, e.accumulated_candidate_model_cost_change = 0;
  else if (e.current_cost > e.candidate_cost) e.candidate_cost = e.current_cost, e.accumulated_candidate_model_cost_change = 0;
  e.reference_cost = e.candidate_cost, e.accumulated_reference_model_cost_change = e.accumulated_candidate_model_cost_change;
  return e;
}

// ComputeTraditionalDoglegStep (CSI/dogleg_strategy.cc:199-255): the step is ca * gradient + cb * gauss_newton, with
// alpha the Cauchy step length and gdot = gradient . gauss_newton. *step_norm is the step's norm where the branch
// knows it, negative where the caller has to take it from the combined step.
VIO_HD void dogleg_combination(double alpha, double gradient_norm, double gauss_newton_norm, double gdot, double radius,
                               double *ca, double *cb, double *step_norm) {
  if (gauss_newton_norm <= radius) {
    *ca = 0, *cb = 1, *step_norm = gauss_newton_norm;
  } else if (gradient_norm * alpha >= radius) {
    *ca = -(radius / gradient_norm), *cb = 0, *step_norm = radius;
  } else {
    const double b_dot_a = -alpha * gdot;
    const double a_squared_norm = pow(alpha * gradient_norm, 2.0);
    const double b_minus_a_squared_norm = a_squared_norm - 2 * b_dot_a + pow(gauss_newton_norm, 2);
    const double c = b_dot_a - a_squared_norm;
    const double d = sqrt(c * c + b_minus_a_squared_norm * (pow(radius, 2.0) - a_squared_norm));
    const double beta = (c <= 0) ? (d - c) / b_minus_a_squared_norm : (radius * radius - a_squared_norm) / (d + c);
    *ca = -alpha * (1.0 - beta), *cb = beta, *step_norm = -1;
  }
}

}  // namespace vio
