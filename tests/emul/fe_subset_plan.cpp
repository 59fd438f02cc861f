// fe_subset_plan.cpp -- drives the front end's subset planner (csrc/fe_subset.h, plain host C++) from a script on stdin, for
// tests/test_frontend_subset_plan.py. First line: the number of sequences. Then one command per line:
//   call  n  seq[0..n)  publish[0..n)  k  frame_index[0..k)     (k = 0: no frame_index; publish "x": a null publish pointer)
//   reset n  seq[0..n)                                          (n = -1: all sequences, a null list)
// and one line of answer each:
//   ok|bad  in_step  bank[0..n_seq)  have[0..n_seq) | seq | slot | prev_bank | forw_bank | publish | pub
#include <stdio.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "fe_subset.h"

int main() {
  int S = 0;
  std::string line;
  if (!std::getline(std::cin, line)) return 2;
  S = std::stoi(line);
  std::vector<uint8_t> bank(S, 0), have(S, 0), seen(S, 0);
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    int n = 0;
    in >> cmd >> n;
    std::vector<int32_t> seq(n > 0 ? n : 0);
    for (auto &s : seq) in >> s;
    seq.reserve(1);  // (an empty list is still a list: data() is not null)
    bool ok = true;
    std::vector<int32_t> arena(fe_subset::arena_ints(n > 0 ? n : 0) + 1, -7);
    fe_subset::Arena A = fe_subset::carve(arena.data(), n > 0 ? n : 0);
    int n_pub = 0;
    if (cmd == "call") {
      std::vector<uint8_t> pub(seq.size());
      bool null_pub = false;
      for (auto &p : pub) {
        std::string t;
        in >> t;
        if (t == "x") null_pub = true;
        else p = (uint8_t)std::stoi(t);
      }
      int k = 0;
      in >> k;
      std::vector<int32_t> fi(k);
      for (auto &f : fi) in >> f;
      const std::vector<uint8_t> bank0 = bank, have0 = have;
      ok = fe_subset::plan(S, bank.data(), have.data(), n, seq.data(), k ? fi.data() : nullptr, -1, null_pub ? nullptr : pub.data(), seen.data(), A,
                           &n_pub);
      if (bank != bank0 || have != have0) return 3;  // plan never writes the phase
      if (ok) fe_subset::commit(bank.data(), have.data(), n, A);
    } else if (cmd == "reset") {
      ok = n < 0 || fe_subset::valid_list(S, n, seq.data(), seen.data());
      if (ok) fe_subset::reset(S, bank.data(), have.data(), n, n < 0 ? nullptr : seq.data());
    } else {
      return 2;
    }
    printf("%s %d", ok ? "ok" : "bad", fe_subset::in_step(S, bank.data(), have.data()) ? 1 : 0);
    for (int s = 0; s < S; s++) printf(" %d", bank[s]);
    for (int s = 0; s < S; s++) printf(" %d", have[s]);
    if (cmd == "call" && ok) {
      const int32_t *rows[6] = {A.seq, A.slot, A.prev_bank, A.forw_bank, A.publish, A.pub};
      for (int r = 0; r < 6; r++) {
        printf(" |");
        for (int i = 0; i < (r == 5 ? n_pub : n); i++) printf(" %d", rows[r][i]);
      }
    }
    printf("\n");
  }
  return 0;
}
