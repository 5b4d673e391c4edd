// tests only: the stand-alone programs of costmap_clusters_host.cpp and costmap_lines_host.cpp (-DCCH_MAIN, -DCLH_MAIN; the sanitizer builds).  A case in the file:
// NHEAD int32 words that begin {B, size_x, size_y, V, O} and hold has_radius, has_velocity at HAS_RADIUS, HAS_RADIUS + 1, double {resolution, behind_robot_dist}, then
// cost, origin, robot_pose and the container as it is before the call (n_obstacles, n_vertices, vertices, [radius], [velocity]).  Its outputs in the other file:
// n_obstacles, n_vertices, vertices, [radius], [velocity], dropped, info.
#pragma once
#include <cstdint>
#include <cstdio>
#include <vector>

template <typename T>
static bool rd(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n; }
template <typename T>
static bool wr(FILE* f, const std::vector<T>& v) { return v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

// the arrays of one case (radius, velocity: NULL when the case has none)
struct CaseArrays {
    const uint8_t* cost; const double* origin; const double* pose;
    int32_t* n_obstacles; int32_t* n_vertices; double* vertices; double* radius; double* velocity; int32_t* dropped; int32_t* info;
};

// call(head, resolution, behind_robot_dist, arrays) on every case of argv[1], the outputs to argv[2]
template <int NHEAD, int HAS_RADIUS, typename Call>
static int run_case_file(int argc, char** argv, const char* name, Call call) {
    if (argc != 3) { std::printf("usage: %s cases outputs\n", argv[0]); return 2; }
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::printf("cannot open the files\n"); return 2; }
    int cases = 0;
    std::vector<int32_t> head;
    while (rd(in, head, NHEAD)) {
        const size_t B = head[0], W = head[1], H = head[2], V = head[3], O = head[4];
        const bool has_rad = head[HAS_RADIUS], has_vel = head[HAS_RADIUS + 1];
        std::vector<double> par, origin, pose, vt, rad, vel;
        std::vector<uint8_t> cost;
        std::vector<int32_t> no, nv, dropped(B, -1), info(4 * B, -1);
        const bool ok = rd(in, par, 2) && rd(in, cost, B * W * H) && rd(in, origin, 2 * B) && rd(in, pose, 3 * B) && rd(in, no, B) && rd(in, nv, B * O) && rd(in, vt, B * O * V * 2) &&
                        rd(in, rad, has_rad ? B * O : 0) && rd(in, vel, has_vel ? B * O * 2 : 0);
        if (!ok) { std::printf("case %d: short read\n", cases); return 2; }
        call(head.data(), par[0], par[1], CaseArrays{cost.data(), origin.data(), pose.data(), no.data(), nv.data(), vt.data(), has_rad ? rad.data() : nullptr,
                                                     has_vel ? vel.data() : nullptr, dropped.data(), info.data()});
        if (!(wr(out, no) && wr(out, nv) && wr(out, vt) && wr(out, rad) && wr(out, vel) && wr(out, dropped) && wr(out, info))) { std::printf("case %d: short write\n", cases); return 2; }
        ++cases;
    }
    std::fclose(in);
    std::fclose(out);
    std::printf("%s: %d cases\n", name, cases);
    return 0;
}
