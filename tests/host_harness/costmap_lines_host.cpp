// tests only: the host build of mpc_local_planner_amd/csrc/mpc_costmap_lines.hpp (the per-instance rule of mpc_costmap_to_lines*) behind a C entry point, in the
// layouts of include/mpc_costmap_lines.h.  No GPU calls.  With -DCLH_MAIN: a stand-alone program that reads cases from a file written by tests/_line_cases.py
// (write_cases), runs them through the same entry point and writes the outputs to another file (the sanitizer build of tests/test_costmap_lines_host.py).
#include "../../mpc_local_planner_amd/csrc/mpc_costmap_lines.hpp"

#include <cmath>
#include <cstdio>
#include <vector>

// B instances through cl_instance; every pointer as in mpc_costmap_to_lines (radius / velocity / dropped / info nullable); prm: {link_dist_sq, inlier_dist_sq,
// min_inliers, n_hypotheses, remaining_outliers}
extern "C" void clh_lines(int B, const uint8_t* cost, int size_x, int size_y, double resolution, const double* origin, const double* robot_pose, double behind_robot_dist,
                          const int32_t* prm, int V, int O, int32_t* n_obstacles, int32_t* n_vertices, double* vertices, double* radius, double* velocity, int32_t* dropped,
                          int32_t* info) {
    const mpc::LineParams lp = {behind_robot_dist, prm[0], prm[1], prm[2], prm[3], prm[4]};
    std::vector<int32_t> lab((size_t)size_x * size_y);
    for (int b = 0; b < B; ++b) {
        const double th = robot_pose[3 * b + 2];
        const mpc::CcMap m = {cost + (size_t)b * size_x * size_y, size_x, size_y, resolution, origin[2 * b], origin[2 * b + 1], robot_pose[3 * b], robot_pose[3 * b + 1], std::cos(th), std::sin(th)};
        const mpc::CcContainer c = {n_vertices + (size_t)b * O, vertices + (size_t)b * O * V * 2, radius ? radius + (size_t)b * O : nullptr, velocity ? velocity + (size_t)b * O * 2 : nullptr};
        mpc::cl_instance(m, lp, V, O, lab.data(), n_obstacles + b, c, dropped ? dropped + b : nullptr, info ? info + 4 * b : nullptr);
    }
}

// the kernel's LDS list capacity, for the tests that straddle it
extern "C" int clh_list_cap() { return mpc::kClListCap; }

#ifdef CLH_MAIN
// A case in the file: int32 {B, size_x, size_y, V, O, has_radius, has_velocity, link_dist_sq, inlier_dist_sq, min_inliers, n_hypotheses, remaining_outliers},
// double {resolution, behind_robot_dist}, then cost, origin, robot_pose and the container as it is before the call (n_obstacles, n_vertices, vertices, [radius],
// [velocity]).  Its outputs in the other file: n_obstacles, n_vertices, vertices, [radius], [velocity], dropped, info.
template <typename T>
static bool rd(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n; }
template <typename T>
static bool wr(FILE* f, const std::vector<T>& v) { return v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char** argv) {
    if (argc != 3) { std::printf("usage: %s cases outputs\n", argv[0]); return 2; }
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::printf("cannot open the files\n"); return 2; }
    int cases = 0;
    std::vector<int32_t> head;
    while (rd(in, head, 12)) {
        const size_t B = head[0], W = head[1], H = head[2], V = head[3], O = head[4];
        std::vector<double> par, origin, pose, vt, rad, vel;
        std::vector<uint8_t> cost;
        std::vector<int32_t> no, nv, dropped(B, -1), info(4 * B, -1);
        const bool ok = rd(in, par, 2) && rd(in, cost, B * W * H) && rd(in, origin, 2 * B) && rd(in, pose, 3 * B) && rd(in, no, B) && rd(in, nv, B * O) && rd(in, vt, B * O * V * 2) &&
                        rd(in, rad, head[5] ? B * O : 0) && rd(in, vel, head[6] ? B * O * 2 : 0);
        if (!ok) { std::printf("case %d: short read\n", cases); return 2; }
        clh_lines((int)B, cost.data(), (int)W, (int)H, par[0], origin.data(), pose.data(), par[1], head.data() + 7, (int)V, (int)O, no.data(), nv.data(), vt.data(),
                  head[5] ? rad.data() : nullptr, head[6] ? vel.data() : nullptr, dropped.data(), info.data());
        if (!(wr(out, no) && wr(out, nv) && wr(out, vt) && wr(out, rad) && wr(out, vel) && wr(out, dropped) && wr(out, info))) { std::printf("case %d: short write\n", cases); return 2; }
        ++cases;
    }
    std::fclose(in);
    std::fclose(out);
    std::printf("costmap_lines_host: %d cases\n", cases);
    return 0;
}
#endif
