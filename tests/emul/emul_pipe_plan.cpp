// TEST INFRASTRUCTURE: the plan of the host-pointer pipeline (babyjubjub-rs_amd/csrc/pipe_plan.hpp) on the CPU, under
// AddressSanitizer / UBSan (tests/test_pipe_plan.py).  One command per line of standard input, one line of output each:
//   plan n n_in n_out in_strides out_strides in_direct out_direct extra first max tail last_on_prio out_at_end pipe_first pipe_chunk env forced parity
//        (lists: comma-separated; forced: the BJJ_PIPE_SCHEDULE string, "-" = unset)  ->  the PipePlan as one JSON object
//   items dflt [string]    pipe_parse_items (no string = the empty string, "NULL" = unset)  ->  the value
//   sched [string]         pipe_parse_schedule  ->  the list, comma-separated in [ ]
//   cap budget per_item pipe_chunk  ->  pipe_super_batch_cap
#include <stdio.h>
#include <string.h>
#include <string>
#include "../../babyjubjub-rs_amd/csrc/pipe_plan.hpp"

static std::vector<size_t> list_of(const char* s) {
  std::vector<size_t> v;
  for (const char* p = s; *p;) { char* q = nullptr; v.push_back((size_t)strtoull(p, &q, 0)); p = *q ? q + 1 : q; }
  return v;
}
static void print_list(const char* key, const size_t* v, size_t n, const char* end) {
  printf("\"%s\":[", key);
  for (size_t i = 0; i < n; i++) printf("%s%zu", i ? "," : "", v[i]);
  printf("]%s", end);
}

int main() {
  char line[4096];
  while (fgets(line, sizeof line, stdin)) {
    std::vector<char*> t;
    for (char* p = strtok(line, " \n"); p; p = strtok(nullptr, " \n")) t.push_back(p);
    if (t.empty()) continue;
    if (!strcmp(t[0], "items") && t.size() >= 2) {
      const char* s = t.size() > 2 ? t[2] : "";
      printf("%zu\n", pipe_parse_items(!strcmp(s, "NULL") ? nullptr : s, (size_t)strtoull(t[1], nullptr, 0)));
    } else if (!strcmp(t[0], "sched")) {
      const std::vector<size_t> v = pipe_parse_schedule(t.size() > 1 ? t[1] : "");
      print_list("sched", v.data(), v.size(), "\n");
    } else if (!strcmp(t[0], "cap") && t.size() == 4) {
      printf("%zu\n", pipe_super_batch_cap(strtoull(t[1], nullptr, 0), strtoull(t[2], nullptr, 0), strtoull(t[3], nullptr, 0)));
    } else if (!strcmp(t[0], "plan") && t.size() == 19) {
      auto num = [&](int k) { return (size_t)strtoull(t[k], nullptr, 0); };
      const int n_in = (int)num(2), n_out = (int)num(3);
      // exactly n_in / n_out entries on the heap: a read past them is the sanitizer's to find
      const std::vector<size_t> is = list_of(t[4]), os = list_of(t[5]), id = list_of(t[6]), od = list_of(t[7]);
      if ((int)is.size() != n_in || (int)id.size() != n_in || (int)os.size() != n_out || (int)od.size() != n_out) { printf("bad lists\n"); return 2; }
      bool* in_direct = new bool[n_in];
      bool* out_direct = new bool[n_out];
      for (int i = 0; i < n_in; i++) in_direct[i] = id[i] != 0;
      for (int i = 0; i < n_out; i++) out_direct[i] = od[i] != 0;
      const std::vector<size_t> forced = pipe_parse_schedule(strcmp(t[17], "-") ? t[17] : nullptr);
      const PipePlan p = pipe_plan({num(1), n_in, n_out, is.data(), os.data(), in_direct, out_direct, num(8), num(9), num(10), num(11), num(12) != 0,
                                    num(13) != 0, num(14), num(15), num(16) != 0, &forced, atoi(t[18])});
      printf("{");
      print_list("lo_of", p.lo_of.data(), p.lo_of.size(), ",");
      printf("\"nchunks\":%zu,\"lane_flip\":%zu,\"max_chunk\":%zu,", p.nchunks(), p.lane_flip, p.max_chunk);
      print_list("d_in_off", p.d_in_off, n_in, ",");
      print_list("d_out_off", p.d_out_off, n_out, ",");
      print_list("r_in_off", p.r_in_off, n_in, ",");
      print_list("r_out_off", p.r_out_off, n_out, ",");
      printf("\"d_extra_off\":%zu,\"dev_tot\":%zu,\"in_ring\":%zu,\"out_ring\":%zu}\n", p.d_extra_off, p.dev_tot, p.in_ring, p.out_ring);
      delete[] in_direct;
      delete[] out_direct;
    } else {
      printf("bad command: %s\n", t[0]);
      return 2;
    }
  }
  return 0;
}
