// Stand-alone host program for tests/test_host_plan_cpu.py: declares the rows of a host-pointer entry point's call in a HostPlan
// (stardis_amd/csrc/sdx_host_plan.h — the very struct the *_f64 entry points fill and HostIo executes), lays it out, binds it to an
// arena of exactly dev_need bytes and writes what came out.  Built by the test with the host compiler; no HIP, no GPU.
//
// Commands on stdin; answers on stdout, text:
//   P staging_max n_rows, then one line per row:
//       i present bytes                     in       (present = 0: the host pointer is null)
//       o present bytes                     out
//       O present pitch row_bytes n_rows    out, 2-D
//       b present bytes back                inout    (back = 0: uploaded only)
//       s bytes                             scratch
//   -> "dev_need pin_need staged", then per row "present dev_off bound width up_off down_off rows uploads downloads": `bound` is the
//      device pointer bind() stored minus the arena's base, -1 for a null pointer; an offset the row does not have is -1
#include <cstdio>
#include <vector>

#include "../stardis_amd/csrc/sdx_host_plan.h"

static long long show(size_t off) { return off == HostPlan::kNone ? -1 : (long long)off; }

int main()
{
    static char host[1];  // every present host pointer (the plan never reads or writes through it)
    char cmd;
    while (std::scanf(" %c", &cmd) == 1) {
        unsigned long long staging_max;
        int n;
        if (cmd != 'P' || std::scanf("%llu %d", &staging_max, &n) != 2 || n < 0) return 2;
        std::vector<const char*> d_in((size_t)n, host);  // (bind() must overwrite every one of these)
        std::vector<char*> d_out((size_t)n, host);
        std::vector<char> kinds((size_t)n);
        HostPlan plan;
        for (int k = 0; k < n; ++k) {
            char kind;
            int present = 1, back = 1;
            unsigned long long bytes = 0, pitch = 0, row_bytes = 0, n_rows = 0;
            if (std::scanf(" %c", &kind) != 1) return 2;
            kinds[(size_t)k] = kind;
            if (kind == 's') {
                if (std::scanf("%llu", &bytes) != 1) return 2;
                plan.scratch((size_t)bytes, &d_out[(size_t)k]);
            } else if (kind == 'O') {
                if (std::scanf("%d %llu %llu %llu", &present, &pitch, &row_bytes, &n_rows) != 4) return 2;
                plan.out2d(present ? host : (char*)nullptr, (size_t)pitch, (size_t)row_bytes, (size_t)n_rows, &d_out[(size_t)k]);
            } else {
                if (std::scanf("%d %llu", &present, &bytes) != 2) return 2;
                if (kind == 'i')
                    plan.in(present ? host : (const char*)nullptr, (size_t)bytes, &d_in[(size_t)k]);
                else if (kind == 'o')
                    plan.out(present ? host : (char*)nullptr, (size_t)bytes, &d_out[(size_t)k]);
                else if (kind == 'b' && std::scanf("%d", &back) == 1)
                    plan.inout(present ? host : (char*)nullptr, (size_t)bytes, &d_out[(size_t)k], back != 0);
                else
                    return 2;
            }
        }
        plan.layout((size_t)staging_max);
        std::vector<char> arena(plan.dev_need + 1);
        plan.bind(arena.data());
        std::printf("%llu %llu %d\n", (unsigned long long)plan.dev_need, (unsigned long long)plan.pin_need, plan.staged ? 1 : 0);
        for (int k = 0; k < n; ++k) {
            const HostPlan::Row& r = plan.rows[(size_t)k];
            const char* bound = kinds[(size_t)k] == 'i' ? d_in[(size_t)k] : d_out[(size_t)k];
            std::printf("%d %lld %lld %llu %lld %lld %llu %d %d\n", r.present ? 1 : 0, show(r.dev_off), bound ? (long long)(bound - arena.data()) : -1,
                        (unsigned long long)r.width(), show(r.up_off), show(r.down_off), (unsigned long long)r.rows, r.uploads() ? 1 : 0, r.downloads() ? 1 : 0);
        }
        std::fflush(stdout);
    }
    return 0;
}
