// The GEMM planner on its own: csrc/gemm_plan.h and nothing else, built with the host compiler under sanitizers by tests/test_gemm_plan_cpu.py.
// stdin: one query per line, the eighteen fields of GemmQuery in order (tests/support_gemm_grid.py); stdout: "<route or FMMT_E*> <workspace bytes or -1>"
// per query, computed the way the entry points of gemm.hip compute them.
#include <stdio.h>
#include "../facialmmt_amd/csrc/gemm_plan.h"

int main() {
    int f[18];
    for (;;) {
        int got = 0;
        while (got < 18 && scanf("%d", &f[got]) == 1) ++got;
        if (got == 0) break;
        if (got < 18) {
            fprintf(stderr, "gemm_plan_sweep: a query of %d fields\n", got);
            return 2;
        }
        const GemmQuery q{f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7], f[8], f[9], f[10] != 0, f[11] != 0, f[12] != 0, f[13] != 0, f[14] != 0, f[15], f[16], f[17]};
        long long ws = -1;
        if (q.mode == GEMM_SPLITK) ws = (long long)plan_query(q).ws_bytes;                        // fmmt_linear_splitk_workspace
        if (q.mode == GEMM_WGRAD || q.mode == GEMM_WGRAD_PARTIALS)                                // fmmt_linear_wgrad_workspace
            ws = q.M <= 0 || q.N <= 0 || q.K <= 0 || (q.dtype != FMMT_BF16 && q.dtype != FMMT_F32) ? 0 : (long long)launch_tn_plan(q).ws_bytes;
        printf("%d %lld\n", route_of(q), ws);
    }
    return 0;
}
