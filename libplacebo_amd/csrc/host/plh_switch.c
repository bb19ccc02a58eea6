/* libplacebo-hip — the one reader of the PL_HIP_* environment switches (hip/plh_switch.h) */
#include <errno.h>
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>

#include "host_common.h"
#include "../hip/plh_switch.h"

static const struct { const char *name; int def; } switches[PLH_SW_COUNT] = {
#define PLH_SWITCH_ROW(id, name, def, doc) { name, def },
    PLH_SWITCHES(PLH_SWITCH_ROW)
#undef PLH_SWITCH_ROW
};

// the variable's value; the default where it is unset, empty or (*bad) no decimal integer from end to end
static int switch_read(int id, bool *bad)
{
    const char *env = getenv(switches[id].name);
    char *end = NULL;
    errno = 0;
    const long v = env && env[0] ? strtol(env, &end, 10) : 0;
    *bad = end && (end == env || *end || errno || v < INT_MIN || v > INT_MAX);
    return end && !*bad ? (int) v : switches[id].def;
}

int plh_switch(enum plh_switch_id id)
{
    bool bad;
    return switch_read(id, &bad);
}

void plh_trace_kernel(const char *name)
{
    if (plh_switch(PLH_SW_PASS_TRACE))
        fprintf(stderr, "[plh] kernel %s\n", name);
}

void plh_switch_report(pl_log log)
{
    static bool warned[PLH_SW_COUNT];
    for (int id = 0; id < PLH_SW_COUNT && log; id++) {
        bool bad;
        const int def = switch_read(id, &bad);
        if (bad && !warned[id])
            pl_msg(log, PL_LOG_WARN, "%s='%s' is not an integer: ignored (default %d)",
                   switches[id].name, getenv(switches[id].name), def);
        warned[id] |= bad;
    }
}
