// Test-only C entries to the any-shape launch plan (plan_any_prod, plan_any_gs, plan_any_update, plan_any_init_chunk:
// lrf_amd/csrc/lrf_plan.cpp) for tests/test_any_plan.py: built with the host compiler, no device.
#include "../lrf_amd/csrc/lrf_plan.h"

enum { PROD_INTS = 12, GS_INTS = 5 };

static void put_prod(const AnyProdPlan& p, long* o)
{
    const long v[PROD_INTS] = {(long)p.k, p.nblk, p.fold, p.tpw, p.tiles, (long)p.gx, (long)p.gy, (long)p.gz, p.threads, (long)p.fold_gx, p.native, p.refused};
    for (int i = 0; i < PROD_INTS; i++) o[i] = v[i];
}
static void put_gs(const AnyGsPlan& g, long* o)
{
    const long v[GS_INTS] = {(long)g.k, (long)g.gx, (long)g.gy, (long)g.lds, g.native_gs};
    for (int i = 0; i < GS_INTS; i++) o[i] = v[i];
}

extern "C" void lrf_test_plan_any_prod(int I, int D, int R, int B, long sai, long sak, int native, int prod_small, long* out)
{
    put_prod(plan_any_prod(I, D, R, B, sai, sak, native != 0, prod_small != 0), out);
}
extern "C" void lrf_test_plan_any_gs(int rows, int R, int B, int int_rows, int gs_f32, long* out)
{
    put_gs(plan_any_gs(rows, R, B, int_rows != 0, gs_f32 != 0), out);
}
// out: the product a, the product b, the sweep
extern "C" void lrf_test_plan_any_update(int B, int M, int N, int R, int trans, int int_rows, int prod_small, int gs_f32, long* out)
{
    const AnyUpdatePlan u = plan_any_update(B, M, N, R, trans != 0, int_rows != 0, prod_small != 0, gs_f32 != 0);
    put_prod(u.a, out);
    put_prod(u.b, out + PROD_INTS);
    put_gs(u.gs, out + 2 * PROD_INTS);
}
extern "C" long lrf_test_plan_any_init_chunk(int n, int Rc, long B) { return plan_any_init_chunk(n, Rc, B); }
