// Stand-alone host program for tests/test_line_geom_cpu.py: runs the launch geometry of the line kernels (stardis_amd/csrc/sdx_line_geom.h —
// the very functions the kernels and the host's launch code use) over every block index and wave of a launch and writes what they return.
// Built by the test with the host compiler; no HIP, no GPU.
//
// Commands on stdin, one per line; answers on stdout, binary, little endian:
//   G nu_begin nu_count n_depth n_split tile_points narrow_f subsets wide_group order mask far_blocks
//       -> int64 {ok, blocks, wide_first, narrow_first}; then, if ok, int32 [narrow_first - wide_first][3] = (tile, depth, live) of every
//          wide-role block and int32 [blocks - narrow_first][n_split][3] = (i0, chunk, live) of every wave of every narrow-role block
//   D d k n_1 .. n_k
//       -> int64 [k]: line_div(n_i, line_div_make(d))
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../stardis_amd/csrc/sdx_line_geom.h"

int main()
{
    char cmd;
    while (std::scanf(" %c", &cmd) == 1) {
        if (cmd == 'G') {
            long long nu_begin, nu_count, far_blocks;
            int n_depth, n_split, tile_points, narrow_f, subsets, wide_group, order, mask;
            if (std::scanf("%lld %lld %d %d %d %d %d %d %d %d %lld", &nu_begin, &nu_count, &n_depth, &n_split, &tile_points, &narrow_f, &subsets, &wide_group, &order,
                           &mask, &far_blocks) != 11)
                return 2;
            const LineLaunch L = line_launch_make(nu_begin, nu_count, n_depth, n_split, tile_points, narrow_f, subsets != 0, wide_group, order, mask, far_blocks);
            const int64_t head[4] = {L.ok ? 1 : 0, L.blocks, L.g.wide_first, L.g.narrow_first};
            std::fwrite(head, sizeof(head), 1, stdout);
            if (L.ok) {
                std::vector<int32_t> out;
                out.reserve((size_t)3 * (size_t)((L.g.narrow_first - L.g.wide_first) + (L.blocks - L.g.narrow_first) * n_split));
                for (int b = L.g.wide_first; b < L.g.narrow_first; ++b) {
                    const WideUnit u = wide_unit(L.g, b);
                    out.push_back(u.tile), out.push_back(u.depth), out.push_back(u.live ? 1 : 0);
                }
                for (int b = L.g.narrow_first; b < (int)L.blocks; ++b)
                    for (int wave = 0; wave < n_split; ++wave) {
                        const NarrowUnit u = subsets ? narrow_unit<true>(L.g, b, wave) : narrow_unit<false>(L.g, b, wave);
                        out.push_back(u.i0), out.push_back(u.chunk), out.push_back(u.live ? 1 : 0);
                    }
                std::fwrite(out.data(), sizeof(int32_t), out.size(), stdout);
            }
        } else if (cmd == 'D') {
            int d, k;
            if (std::scanf("%d %d", &d, &k) != 2) return 2;
            const LineDiv v = line_div_make(d);
            std::vector<int64_t> q((size_t)k);
            for (int i = 0; i < k; ++i) {
                int n;
                if (std::scanf("%d", &n) != 1) return 2;
                q[(size_t)i] = line_div(n, v);
            }
            std::fwrite(q.data(), sizeof(int64_t), q.size(), stdout);
        } else {
            return 2;
        }
        std::fflush(stdout);
    }
    return 0;
}
