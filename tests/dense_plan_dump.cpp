// Prints csrc/dense_plan.h -- the schedule the fused dense-block kernels are compiled from -- as one JSON object, for tests/dense_plan.py.
// Built with the host compiler alone: g++ -std=c++17 -I <csrc> dense_plan_dump.cpp
#include <cstdio>

#include "dense_plan.h"

using namespace dense_plan;

template <class F> static void arr(int n, F&& f) {
    printf("[");
    for (int i = 0; i < n; ++i) { if (i) printf(","); f(i); }
    printf("]");
}
template <class F> static void list(const char* key, int n, F&& f, const char* end = ",") {
    printf("\"%s\":", key);
    arr(n, f);
    printf("%s", end);
}
static void num(int v) { printf("%d", v); }

template <int EXT, int NB0, int NB1, int MODE, int LW> static void loader() {
    using P = LoaderPlan<EXT, NB0, NB1, MODE, LW>;
    printf("{");
    list("rows", 3, [](int kx) { arr(P::nrows(kx), [&](int r) { num(P::row(kx, r)); }); });
    list("nst_at", P::NGR, [](int i) { num(P::nst_at(i)); });
    list("resident", P::NGR, [](int iw) { arr(P::npieces(iw), [&](int k) { num(P::resident(iw, k)); }); });
    list("nwdma", P::NGR, [](int iw) { num(P::nwdma(iw)); });
    list("issue_w", P::NGR, [](int i) { num(P::issue_w(i)); });
    list("wait_rows", P::NGR, [](int i) { num(P::wait_rows(i)); });
    list("wait_n", P::NGR, [](int i) { num(P::wait_n(i)); }, "");
    printf("}");
}

template <int EXT, int MODE, bool CARRY> static void carry(const char* key) {
    using C = CarryPlan<EXT, MODE, CARRY>;
    printf("\"%s\":{", key);
    list("pre_w", C::NGR, [](int i) { num(C::pre_w(i)); });
    list("pre_x", C::NGR, [](int i) { num(C::pre_x(i)); });
    list("npre", C::NGR, [](int i) { num(C::npre(i)); }, "");
    printf("},");
}

template <int EXT, int NB0, int NB1, int MODE> static void shape(const char* end) {
    using L = ChainLds<NB0, NB1, MODE>;
    using P = LoaderPlan<EXT, NB0, NB1, MODE, 0>;
    printf("\"%d,%d,%d,%d\":{", EXT, NB0, NB1, MODE);
    printf("\"extg\":%d,\"ngr\":%d,\"rt_e\":%d,\"rt_r\":%d,\"wl\":%d,\"sl\":%d,", P::EXTG, P::NGR, P::RT_E, P::RT_R, P::WL, P::SL);
    printf("\"lds\":{\"nsb\":%d,\"nws\":%d,\"wslot\":%d,\"bytes\":%d},", L::NSB, L::NWS, L::WSLOT, L::BYTES);
    list("npieces", P::NGR, [](int iw) { num(P::npieces(iw)); });
    printf("\"loaders\":[");
    loader<EXT, NB0, NB1, MODE, 0>(); printf(",");
    loader<EXT, NB0, NB1, MODE, 1>(); printf(",");
    loader<EXT, NB0, NB1, MODE, 2>(); printf(",");
    loader<EXT, NB0, NB1, MODE, 3>(); printf("],");
    carry<EXT, MODE, kCarry<MODE>>("carry");                   // what the kernel is built with
    carry<EXT, MODE, true>("carry_forced");                    // the plan switched on regardless (the growth pairs' negative test)
    list("ext_stages", ext_stages(NB0, NB1), [](int k) { const ExtStage s = ext_stage(NB0, NB1, k); printf("[%d,%d,%d,%d]", s.d, s.layer, s.n, s.first); });
    list("ring_stages", ring_stages(NB1), [](int k) { const RingStage s = ring_stage(NB1, k); printf("[%d,%d]", s.ky, s.n); });
    list("frags", nfrags(EXT, NB0, NB1), [](int f) { const Frag r = frag_at(EXT, NB0, NB1, f); printf("[%d,%d,%d,%d,%d]", r.conv, r.chunk, r.ky, r.kx, r.blk); }, "");
    printf("}%s", end);
}

template <int LW> static void conv1_loader(const char* end) {
    using P = Conv1LoaderPlan<LW>;
    printf("{\"np\":%d,\"ahead\":%d,\"wait\":%d,", P::NP, P::AHEAD, P::WAIT);
    list("rows", P::NROWS, [](int r) { num(P::row(r)); }, "");
    printf("}%s", end);
}

int main() {
    printf("{\"ROWB\":%d,\"NSTG\":%d,\"WINR\":%d,\"NCOMP\":%d,\"NLOAD\":%d,\"WDEPTH\":%d,\"NWQ\":%d,", ROWB, NSTG, WINR, NCOMP, NLOAD, WDEPTH, NWQ);
    printf("\"shapes\":{");
    shape<5, 2, 4, 1>(",");
    shape<2, 2, 2, 0>(",");
    shape<3, 2, 2, 0>("},");
    printf("\"conv1\":{\"nstg\":%d,\"nsb\":%d,\"wbytes\":%d,\"lds\":%d,\"loaders\":[", C1_NSTG, C1_NSB, C1_WBYTES, C1_LDS);
    conv1_loader<0>(","); conv1_loader<1>(","); conv1_loader<2>(","); conv1_loader<3>("]}}\n");
    return 0;
}
