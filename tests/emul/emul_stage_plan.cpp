// TEST INFRASTRUCTURE: the layout of a staged host call (babyjubjub-rs_amd/csrc/stage_plan.hpp) on the CPU, under AddressSanitizer /
// UBSan (tests/test_stage_plan.py).  One plan per line of standard input, one line of output each:
//   prefix round_last array...      array = i:count:width | o:count:width (behind what is there) | I:offset:bytes | O:offset:bytes (at an
//                                   offset inside the prefix)
//   ->  {"idx":[...],"off":[...],"bytes":[...],"out":[...],"total":T}     idx: what the declaration returned (-1 = the plan was full)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../babyjubjub-rs_amd/csrc/stage_plan.hpp"

int main() {
  char line[4096];
  while (fgets(line, sizeof line, stdin)) {
    std::vector<char*> t;
    for (char* p = strtok(line, " \n"); p; p = strtok(nullptr, " \n")) t.push_back(p);
    if (t.size() < 2) { printf("bad line\n"); return 2; }
    StagePlan* plan = new StagePlan((size_t)strtoull(t[0], nullptr, 0));   // on the heap: a write past a[] is the sanitizer's to find
    const bool round_last = atoi(t[1]) != 0;
    std::vector<int> idx;
    for (size_t k = 2; k < t.size(); k++) {
      char kind = 0;
      unsigned long long a = 0, b = 0;
      if (sscanf(t[k], "%c:%llu:%llu", &kind, &a, &b) != 3 || !strchr("ioIO", kind)) { printf("bad array: %s\n", t[k]); return 2; }
      const bool out = kind == 'o' || kind == 'O';
      idx.push_back(kind == 'i' || kind == 'o' ? plan->add(out, (size_t)a, (size_t)b) : plan->at(out, (size_t)a, (size_t)b));
    }
    printf("{\"idx\":[");
    for (size_t i = 0; i < idx.size(); i++) printf("%s%d", i ? "," : "", idx[i]);
    const char* keys[3] = {"off", "bytes", "out"};
    for (int f = 0; f < 3; f++) {
      printf("],\"%s\":[", keys[f]);
      for (int i = 0; i < plan->n; i++) printf("%s%zu", i ? "," : "", f == 0 ? plan->a[i].off : f == 1 ? plan->a[i].bytes : (size_t)plan->a[i].out);
    }
    printf("],\"total\":%zu}\n", plan->total(round_last));
    delete plan;
  }
  return 0;
}
