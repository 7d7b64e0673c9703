/* The transformed-nest entry points of include/xpoly_amd.h as C99: takes the address of each through its prototype and asks
 * the host-only plan view (no device is opened). Prints the ten figures of the plan of 65 nests of 6 x 4 at depth 3. */
#include <stdio.h>
#include "xpoly_amd.h"

int main(void)
{
    int (*packed)(xpg_ctx *, int, const xpg_rat32 *, int, const xpg_rat32 *, int, int, int, int, int, int, xpg_rat32 *, long long,
                  const xpg_rat32 **, long long *, int32_t *, int32_t *, int32_t *, xpg_rat32 *, xpg_rat32 *) =
        xpg_lineq_transform_levels_batch_packed_rat32;
    int (*dev)(xpg_ctx *, int, const xpg_rat32 *, int, const xpg_rat32 *, int, int, int, int, int, int, xpg_rat32 *, int32_t *, int32_t *,
               int32_t *, int32_t *, xpg_rat32 *, xpg_rat32 *) = xpg_lineq_transform_levels_batch_rat32_dev;
    int (*route)(long long *, int) = xpg_lineq_transform_last_route;
    long long f[10];
    int k;
    if (!packed || !dev || !route) return 1;
    if (xpg_test_lineq_transform_plan(65, 6, 4, 3, 0, 0, f, 10) != 0) return 1;
    for (k = 0; k < 10; k++) printf("%lld ", f[k]);
    printf("\n");
    return 0;
}
