// tests/emul/solve_trace_check.cpp — TEST-ONLY driver of vins-mobile_amd/csrc/solve_trace.h on the host
// (tests/test_solve_trace.py): runs one piece on the numbers of its command line and prints what came out, %.17g.
//   trace N R            N record calls (i = 0 .. N-1) into raw arrays pre-filled with NaN / -1, finish(recorded = R),
//                        unpack_solve_stats; prints every field of the VioSolveStats and whether the guards behind the
//                        raw arrays are intact
//   evaluator C0 {C M}   StepEvaluator::at(C0); per pair: rho of a step to cost C with model cost change M, the step
//                        accepted, the six members afterwards
//   dogleg A G N D R     dogleg_combination(alpha, gradient_norm, gauss_newton_norm, gdot, radius): ca cb step_norm
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <limits>
#include <vector>

#include "solve_trace.h"

using namespace vio;

// what record i holds: the test computes the same numbers
static double rec_cost(int i) { return 100.0 - i; }
static double rec_radius(int i) { return 1e4 / (1 + i); }
static double rec_step_norm(int i) { return 0.25 * i; }
static double rec_rel(int i) { return 0.5 + 0.125 * i; }
static double rec_gmax(int i) { return 1.0 / (1 + i); }

template <class T>
static void print_array(const char *name, const T *a, const char *fmt) {
  printf("%s", name);
  for (int i = 0; i < VIO_MAX_TRACE; i++) printf(" "), printf(fmt, a[i]);
  printf("\n");
}

int main(int argc, char **argv) {
  if (argc >= 4 && !strcmp(argv[1], "trace")) {
    const int n = atoi(argv[2]), recorded = atoi(argv[3]);
    std::vector<double> sd(kStatsDoubles + 1, std::numeric_limits<double>::quiet_NaN());
    std::vector<int> si(kStatsInts + 1, -1);
    sd[kStatsDoubles] = 12345.0, si[kStatsInts] = 12345;
    const SolveTrace trace{sd.data(), si.data()};
    trace.initial(rec_cost(0));
    for (int i = 0; i < n; i++) trace.record(i, rec_cost(i), rec_radius(i), rec_step_norm(i), rec_rel(i), rec_gmax(i), i % 2 == 0, i % 3 == 0);
    trace.finish(recorded, 1, 7, 3, 36.5);
    VioSolveStats st;
    memset(&st, 0xff, sizeof(st));
    unpack_solve_stats(sd.data(), si.data(), &st);
    printf("guards %d\n", sd[kStatsDoubles] == 12345.0 && si[kStatsInts] == 12345);
    printf("header %.17g %.17g %d %d %d %d\n", st.initial_cost, st.final_cost, st.iterations, st.termination, st.num_successful_steps,
           st.num_unsuccessful_steps);
    print_array("it_cost", st.it_cost, "%.17g");
    print_array("it_radius", st.it_radius, "%.17g");
    print_array("it_step_norm", st.it_step_norm, "%.17g");
    print_array("it_relative_decrease", st.it_relative_decrease, "%.17g");
    print_array("it_gradient_max_norm", st.it_gradient_max_norm, "%.17g");
    print_array("it_flags", st.it_flags, "%d");
    return 0;
  }
  if (argc >= 3 && !strcmp(argv[1], "evaluator")) {
    StepEvaluator ev = StepEvaluator::at(atof(argv[2]));
    for (int k = 3; k + 1 < argc; k += 2) {
      const double cost = atof(argv[k]), model_cost_change = atof(argv[k + 1]);
      const double rho = step_quality(ev, cost, model_cost_change);
      ev = step_accepted(ev, cost, model_cost_change);
      printf("%.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", rho, ev.minimum_cost, ev.current_cost, ev.reference_cost, ev.candidate_cost,
             ev.accumulated_reference_model_cost_change, ev.accumulated_candidate_model_cost_change);
    }
    return 0;
  }
  if (argc == 7 && !strcmp(argv[1], "dogleg")) {
    double ca = 99, cb = 99, step_norm = 99;
    dogleg_combination(atof(argv[2]), atof(argv[3]), atof(argv[4]), atof(argv[5]), atof(argv[6]), &ca, &cb, &step_norm);
    printf("%.17g %.17g %.17g\n", ca, cb, step_norm);
    return 0;
  }
  fprintf(stderr, "usage: %s trace N R | evaluator C0 {C M} | dogleg A G N D R\n", argv[0]);
  return 2;
}
