// plan_dump: the GEMM / conv planner (cremage_amd/csrc/gemm_plan.h) without a device.  Reads rows of the route table on stdin
// (tests/routes/parent_routes.jsonl, one JSON object per line as tools/record_routes.py writes them), rebuilds the args - a pointer
// field becomes a fake address of the recorded alignment, the planner never dereferences one - and prints, per row,
//
//     rc kernel wnt config splits tail_splits rowhalo halo_lin pair up2 mx reduce gn_stats_rows [| message]
//
// Dev knobs are the defaults; tune_samples and n_cu are the row's.
//     c++ -std=c++17 -Wall -Werror -fsanitize=address,undefined tools/plan_dump.cpp -o plan_dump && ./plan_dump < tests/routes/parent_routes.jsonl
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>

#include "../cremage_amd/csrc/gemm_plan.h"

namespace {

// the text of field `key`'s value in `obj` ("" when absent): the whole row for its top-level fields (fn, tune_samples, n_cu), the "args"
// object (args_of) for the args, whose names would otherwise collide with the route's (gn_stats_rows is in both)
std::string raw(const std::string& row, const char* key) {
  const std::string pat = std::string("\"") + key + "\":";
  size_t i = row.find(pat);
  if (i == std::string::npos) return "";
  i += pat.size();
  while (i < row.size() && row[i] == ' ') ++i;
  size_t j = i;
  if (row[i] == '[') j = row.find(']', i) + 1;
  else if (row[i] == '"') j = row.find('"', i + 1) + 1;
  else while (j < row.size() && row[j] != ',' && row[j] != '}') ++j;
  return row.substr(i, j - i);
}

// the "args" object of a row: it holds arrays but no nested object, so it ends at the first closing brace
std::string args_of(const std::string& row) {
  const size_t i = row.find("\"args\":");
  if (i == std::string::npos) return "";
  const size_t a = row.find('{', i), b = row.find('}', i);
  return a == std::string::npos || b == std::string::npos ? "" : row.substr(a, b - a + 1);
}

long num(const std::string& row, const char* key) { return strtol(raw(row, key).c_str(), nullptr, 10); }
float real(const std::string& row, const char* key) { return strtof(raw(row, key).c_str(), nullptr); }

// "null" -> nullptr, an address mod 16 -> a fake address of that alignment
template <typename T>
T* ptr(const std::string& row, const char* key) {
  const std::string v = raw(row, key);
  if (v.empty() || v == "\"null\"") return nullptr;
  return reinterpret_cast<T*>((uintptr_t)0x100000 + (uintptr_t)strtol(v.c_str(), nullptr, 10));
}

crg_gemm_args gemm_args(const std::string& r) {
  crg_gemm_args a{};
  a.a = ptr<void>(r, "a"); a.lda = num(r, "lda"); a.a_bstride = num(r, "a_bstride");
  a.w = ptr<void>(r, "w"); a.ldw = num(r, "ldw"); a.w_bstride = num(r, "w_bstride");
  a.w_lo = ptr<void>(r, "w_lo");
  a.bias = ptr<float>(r, "bias"); a.bias_mode = (int)num(r, "bias_mode");
  a.residual = ptr<void>(r, "residual"); a.ldr = num(r, "ldr"); a.r_bstride = num(r, "r_bstride");
  a.y = ptr<void>(r, "y"); a.ldy = num(r, "ldy"); a.y_bstride = num(r, "y_bstride");
  a.M = (int)num(r, "M"); a.N = (int)num(r, "N"); a.K = (int)num(r, "K"); a.batch = (int)num(r, "batch");
  a.epilogue = (int)num(r, "epilogue");
  a.a_dtype = (int)num(r, "a_dtype"); a.y_dtype = (int)num(r, "y_dtype"); a.prec = (int)num(r, "prec");
  a.a_is_weight = (int)num(r, "a_is_weight");
  a.a_lo = ptr<void>(r, "a_lo");
  a.gn_stats = ptr<float>(r, "gn_stats");
  a.vt = ptr<void>(r, "vt"); a.vt_n0 = (int)num(r, "vt_n0"); a.vt_tokens = (int)num(r, "vt_tokens"); a.vt_ld = num(r, "vt_ld");
  a.row_stats = ptr<float>(r, "row_stats"); a.row_stats_parts = (int)num(r, "row_stats_parts");
  a.ln_stats = ptr<float>(r, "ln_stats"); a.ln_parts = (int)num(r, "ln_parts"); a.ln_colsum = ptr<float>(r, "ln_colsum"); a.ln_eps = real(r, "ln_eps");
  a.rows_per_sample = (int)num(r, "rows_per_sample");
  return a;
}

crg_conv_args conv_args(const std::string& r, int* rows_out) {
  crg_conv_args a{};
  a.x = ptr<void>(r, "x"); a.x2 = ptr<void>(r, "x2"); a.C1 = (int)num(r, "C1"); a.C2 = (int)num(r, "C2");
  a.w = ptr<void>(r, "w"); a.w_lo = ptr<void>(r, "w_lo");
  a.bias = ptr<float>(r, "bias"); a.cvec = ptr<float>(r, "cvec");
  a.cvec_ld = num(r, "cvec_ld");
  a.residual = ptr<void>(r, "residual");
  a.y = ptr<void>(r, "y");
  a.N = (int)num(r, "N"); a.H = (int)num(r, "H"); a.W = (int)num(r, "W"); a.Cout = (int)num(r, "Cout"); a.Ho = (int)num(r, "Ho"); a.Wo = (int)num(r, "Wo");
  a.ksize = (int)num(r, "ksize"); a.stride = (int)num(r, "stride"); a.pad_t = (int)num(r, "pad_t"); a.pad_l = (int)num(r, "pad_l");
  a.upsample2x = (int)num(r, "upsample2x");
  a.x_dtype = (int)num(r, "x_dtype"); a.y_dtype = (int)num(r, "y_dtype"); a.prec = (int)num(r, "prec");
  a.x_lo = ptr<void>(r, "x_lo");
  a.gn_stats = ptr<float>(r, "gn_stats");
  a.gn_gamma = ptr<float>(r, "gn_gamma"); a.gn_beta = ptr<float>(r, "gn_beta"); a.gn_y = ptr<void>(r, "gn_y");
  a.gn_groups = (int)num(r, "gn_groups"); a.gn_silu = (int)num(r, "gn_silu"); a.gn_eps = real(r, "gn_eps");
  const std::string mx = raw(r, "mx_log2");  // [a, b, c, d]
  if (mx.size() > 1) {
    const char* s = mx.c_str() + 1;
    for (int i = 0; i < 4; ++i) {
      char* end = nullptr;
      a.mx_log2[i] = (int)strtol(s, &end, 10);
      s = *end ? end + 1 : end;
    }
  }
  a.gn_stats_rows = raw(r, "gn_stats_rows") == "\"null\"" ? nullptr : rows_out;
  return a;
}

}  // namespace

int main() {
  std::string row;
  while (std::getline(std::cin, row)) {
    if (row.empty()) continue;
    crg_plan::Env env;
    env.tune_samples = (int)num(row, "tune_samples");
    env.n_cu = (int)num(row, "n_cu");
    int rows_out = 0;
    const std::string fn = raw(row, "fn");
    crg_plan::Plan pl;
    const std::string args = args_of(row);
    if (fn == "\"gemm\"") pl = crg_plan::plan_gemm(gemm_args(args), env);
    else if (fn == "\"conv\"") pl = crg_plan::plan_conv(conv_args(args, &rows_out), env);
    else {
      std::cerr << "plan_dump: a row that is neither gemm nor conv: " << row.substr(0, 80) << "\n";
      return 2;
    }
    const crg_route r = pl.rc ? crg_route{} : pl.route;  // (a refused call leaves the record cleared)
    std::cout << pl.rc << ' ' << r.kernel << ' ' << r.wnt << ' ' << r.config << ' ' << r.splits << ' ' << r.tail_splits << ' ' << r.rowhalo << ' '
              << r.halo_lin << ' ' << r.pair << ' ' << r.up2 << ' ' << r.mx << ' ' << r.reduce << ' ' << r.gn_stats_rows;
    if (pl.rc) std::cout << " | " << pl.msg;
    std::cout << '\n';
  }
  return 0;
}
