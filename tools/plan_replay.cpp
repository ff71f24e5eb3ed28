// The conv planner on its own: csrc/conv_plan.cpp compiled by a plain host compiler (no HIP headers)
// and linked with a stub device_cus(), replaying launches of tests/golden/conv_plans.json.
//
//   python tools/plan_table.py --dump-text tests/golden/conv_plans.json 64 > /tmp/plans.txt
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tools/plan_replay.cpp
//       speech-to-video-mpp_amd/csrc/conv_plan.cpp -o /tmp/plan_replay        (one command line)
//   /tmp/plan_replay /tmp/plans.txt
//
// Input, one launch per line: "field=value ... | rc ws out0 .. out10" (the ints of a failed plan omitted).
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <sstream>
#include <string>

#include "../speech-to-video-mpp_amd/csrc/conv_plan.hpp"

namespace s2v {
static char g_err[512];
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
int device_cus() { return 0; }
}  // namespace s2v

#define F(name, type) {#name, {offsetof(s2v_conv_params, name), type}}
enum { I, LL, FL, PTR };
static const std::map<std::string, std::pair<size_t, int>> kFields = {
    F(x, PTR), F(n, I), F(h, I), F(w, I), F(cin, I), F(xcs, I), F(in_mode, I), F(pad_mode, I), F(pre_act, I),
    F(pre_alpha, FL), F(in_scale, PTR), F(in_scale_ns, I), F(kh, I), F(kw, I), F(sh, I), F(sw, I), F(ph, I), F(pw, I),
    F(dh, I), F(dw, I), F(wt, PTR), F(kpad, I), F(npad, I), F(cout, I), F(b_kn, I), F(ldb, I), F(y, PTR), F(oh, I),
    F(ow, I), F(ycs, I), F(scale, PTR), F(shift, PTR), F(nc_scale, PTR), F(nc_scale_ns, I), F(pix_add, PTR),
    F(pix_w, FL), F(res, PTR), F(res_cs, I), F(res_h, I), F(res_w, I), F(res_oy, I), F(res_ox, I),
    F(res_after_act, I), F(act, I), F(alpha, FL), F(batch, I), F(x_bs, LL), F(w_bs, LL), F(y_bs, LL), F(res_bs, LL),
    F(force_tile, I), F(force_splits, I), F(out_step, I), F(out_full_h, I), F(out_full_w, I), F(prec, I),
    F(wt_x3, PTR), F(grid_cap, I), F(wt_scale, FL), F(out_pool, I), F(x_split, I), F(x_scale, FL), F(d2s_cout, I),
    F(post_mul, PTR), F(post_add, PTR), F(post_cs, I), F(post_c0, I), F(dup_src, PTR), F(dup_bias, PTR),
    F(dup_a, FL), F(dup_cs, I), F(dup_off, I)};

int main(int argc, char **argv) {
    FILE *f = argc > 1 ? fopen(argv[1], "r") : nullptr;
    if (!f) return fprintf(stderr, "usage: plan_replay FILE\n"), 2;
    char line[4096];
    int n = 0, bad = 0;
    while (fgets(line, sizeof(line), f)) {
        s2v_conv_params p{};
        std::istringstream in(line);
        std::string tok;
        while (in >> tok && tok != "|") {
            const size_t eq = tok.find('=');
            const auto it = kFields.find(tok.substr(0, eq));
            if (eq == std::string::npos || it == kFields.end()) return fprintf(stderr, "bad field %s\n", tok.c_str()), 2;
            char *dst = (char *)&p + it->second.first;
            const char *v = tok.c_str() + eq + 1;
            switch (it->second.second) {
                case I: *(int *)dst = atoi(v); break;
                case LL: *(long long *)dst = atoll(v); break;
                case FL: *(float *)dst = (float)atof(v); break;
                default: *(uintptr_t *)dst = (uintptr_t)strtoull(v, nullptr, 10); break;
            }
        }
        long long want_rc, want_ws;
        in >> want_rc >> want_ws;
        s2v::Plan pl;
        const int rc = s2v::plan_conv(&p, pl);
        int out[11] = {0};
        bool ok = rc == want_rc && (rc != 0 || (long long)pl.ws_bytes == want_ws);
        if (rc == 0) {
            s2v::encode_plan(pl, out);
            for (int i = 0, w; i < 11 && (in >> w); ++i) ok = ok && w == out[i];
        }
        ++n;
        if (!ok) {
            ++bad;
            fprintf(stderr, "line %d: rc %d (%s), ws %zu, plan %d %d %d %d %d %d\n", n, rc, rc ? s2v::g_err : "ok", pl.ws_bytes,
                    out[0], out[1], out[2], out[3], out[4], out[5]);
        }
    }
    fclose(f);
    printf("%d launches replayed, %d mismatches\n", n, bad);
    return bad != 0;
}
