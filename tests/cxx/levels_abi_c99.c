/* Compiled as C99 by tests/test_lineq_levels_host.py: the prototypes of the levels entry points must be plain C. Every one is
 * bound through a pointer of its declared type; the host-only plan view is asked (no device is opened) and its nine figures
 * printed on one line. */
#include "xpoly_amd.h"
#include <stdio.h>

typedef int (*packed_fn)(xpg_ctx *, int, const xpg_rat32 *, int, int, int, const int32_t *, int, int, int, int, xpg_rat32 *, long long,
                         const xpg_rat32 **, long long *, int32_t *, int32_t *);
typedef int (*dev_fn)(xpg_ctx *, int, const xpg_rat32 *, int, int, int, const int32_t *, int, int, int, int, xpg_rat32 *, int32_t *,
                      int32_t *, int32_t *);
typedef int (*route_fn)(long long *, int);
typedef int (*plan_fn)(int, int, int, int, int, int, long long *, int);

int main(void)
{
    packed_fn packed = xpg_lineq_levels_batch_packed_rat32;
    dev_fn dev = xpg_lineq_levels_batch_rat32_dev;
    route_fn route = xpg_lineq_levels_last_route;
    plan_fn plan = xpg_test_lineq_levels_plan;
    long long f[9];
    int k;
    if (!packed || !dev || !route) return 1;
    if (plan(48, 9, 5, 3, 256, 0, f, 9) != 0) return 1;
    for (k = 0; k < 9; k++) printf("%lld%c", f[k], k == 8 ? '\n' : ' ');
    return 0;
}
