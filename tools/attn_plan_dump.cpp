// attn_plan_dump: the attention planner (cremage_amd/csrc/attention_plan.h) without a device.  Reads one JSON object per line on stdin,
//
//     {"B": 2, "H": 8, "Nq": 4096, "Nk": 77, "Dh": 40, "ldk": 320, "ldv": 80, "vrm": 0, "samples": 2, "ctx": 1, "dma": 1, "tail": 1, "occ4": 1}
//
// (ldk / ldv in elements; samples: the heuristic sample count, B unless the batch-invariant mode is on; the four knobs may be left out:
// defaults) and prints, per line,
//
//     rc family kk nv ones vrm nw occ sub grid_x grid_y threads [| message]
//
// with kk = KS for the reg / ctx families and KC for dma / sp.  --list prints every dispatchable variant, `family kk nv ones vrm nw occ sub`.
//     c++ -std=c++17 -Wall -Werror -fsanitize=address,undefined tools/attn_plan_dump.cpp -o attn_plan_dump && ./attn_plan_dump --list
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>

#include "../cremage_amd/csrc/attention_plan.h"

namespace {

// the integer value of top-level field `key` of `row` (the rows hold numbers only), or `dflt` when absent
long num(const std::string& row, const char* key, long dflt) {
  const std::string pat = std::string("\"") + key + "\":";
  size_t i = row.find(pat);
  if (i == std::string::npos) return dflt;
  i += pat.size();
  while (i < row.size() && row[i] == ' ') ++i;
  return strtol(row.c_str() + i, nullptr, 10);
}

void print_variant(const crg_attn_plan::Variant& v) {
  std::cout << crg_attn_plan::family_name(v.family) << ' ' << v.kk << ' ' << v.nv << ' ' << v.ones << ' ' << v.vrm << ' ' << v.nw << ' ' << v.occ << ' '
            << v.sub;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1) {
    if (argc != 2 || strcmp(argv[1], "--list") != 0) {
      std::cerr << "usage: attn_plan_dump [--list] < rows.jsonl\n";
      return 2;
    }
    for (const crg_attn_plan::Variant& v : crg_attn_plan::VARIANTS) {
      print_variant(v);
      std::cout << '\n';
    }
    return 0;
  }
  std::string row;
  while (std::getline(std::cin, row)) {
    if (row.empty()) continue;
    crg_attn_plan::Knobs kn;
    kn.ctx = (int)num(row, "ctx", kn.ctx);
    kn.dma = (int)num(row, "dma", kn.dma);
    kn.tail = (int)num(row, "tail", kn.tail);
    kn.occ4 = (int)num(row, "occ4", kn.occ4);
    const int B = (int)num(row, "B", 0);
    const crg_attn_plan::Plan pl =
        crg_attn_plan::plan_attention(B, (int)num(row, "H", 0), (int)num(row, "Nq", 0), (int)num(row, "Nk", 0), (int)num(row, "Dh", 0), num(row, "ldk", 0),
                                      num(row, "ldv", 0), num(row, "vrm", 0) != 0, num(row, "samples", B), kn);
    std::cout << pl.rc << ' ';
    if (pl.rc || pl.variant < 0) std::cout << "none 0 0 0 0 0 0 0";
    else print_variant(crg_attn_plan::VARIANTS[pl.variant]);
    std::cout << ' ' << pl.grid_x << ' ' << pl.grid_y << ' ' << pl.threads;
    if (pl.rc) std::cout << " | " << pl.msg;
    std::cout << '\n';
  }
  return 0;
}
