// tests only: the host build of mpc_local_planner_amd/csrc/mpc_costmap_scans.hpp (the per-instance rule of mpc_costmap_scans*) behind a C entry point, in the
// layouts of include/mpc_costmap_scans.h.  No GPU calls.  With -DCSH_MAIN: a stand-alone program that reads cases from a file written by tests/_scan_cases.py
// (write_cases), runs them through the same entry point and writes the outputs to another file (the sanitizer build of tests/test_costmap_scans_host.py).
#include "../../mpc_local_planner_amd/csrc/mpc_costmap_scans.hpp"
#include "../../mpc_local_planner_amd/csrc/mpc_costmap_window.hpp"

#include <cstdio>
#include <vector>

// B instances through cs_instance.  dpar: {lattice_anchor x, y, sensor_pose x, y, yaw, angle_min, angle_increment, range_min, range_max, obstacle_range, raytrace_range,
// footprint_clear_radius}; ipar: {marking, clearing, inf_is_valid, track_unknown, combination_method}; keep [B], cost [B][size_y][size_x] and info [B][4] nullable.
// Returns rule 4's R, -1 when it is above the limit (nothing is written then).
extern "C" int csh_scans(int B, const double* dpar, const int32_t* ipar, const double* robot_pose, const float* ranges, int n_beams, const int32_t* keep, int size_x,
                         int size_y, double resolution, uint8_t* layer, int32_t* layer_cell, uint8_t* cost, int32_t* info) {
    const int R = mpc::cs_ray_cells(dpar[10], resolution);
    if (R < 0) return -1;
    const mpc::ScanParams p = {dpar[0], dpar[1], resolution, dpar[2], dpar[3], dpar[4], dpar[5], dpar[6], dpar[7], dpar[8], dpar[9], dpar[11],
                               ipar[0] ? 1 : 0, ipar[1] ? 1 : 0, ipar[2] ? 1 : 0, ipar[4], R, ipar[3] ? 255 : 0};
    const size_t cells = (size_t)size_x * size_y;
    for (int b = 0; b < B; ++b)
        mpc::cs_instance(p, robot_pose + 3 * (size_t)b, ranges + (size_t)b * n_beams, n_beams, keep && keep[b] != 0, size_x, size_y, layer + b * cells,
                         layer_cell + 2 * (size_t)b, cost ? cost + b * cells : nullptr, info ? info + 4 * (size_t)b : nullptr);
    return R;
}

// the pieces of the rule on their own
extern "C" void csh_sincos(double x, double* sn, double* cs) { mpc::cs_sincos(x, *sn, *cs); }
extern "C" double csh_wrap(double x) { return mpc::cs_wrap(x); }
extern "C" int csh_steps(int dx, int dy, int R) { return mpc::cs_steps(dx, dy, R); }
// rule 1 against the window's: 1 when both refuse, or both accept and give the same origin; *cell: the index the scans' keeps
extern "C" int csh_origin_agrees(double pose, int size, double res, double anchor, double* origin, int32_t* cell) {
    double mine = 0.0, theirs = 0.0;
    const bool a = mpc::cs_origin_axis(pose, size, res, anchor, mine, *cell), b = mpc::cw_origin_axis(pose, size, res, anchor, theirs);
    *origin = mine;
    return a == b && (!a || __builtin_memcmp(&mine, &theirs, 8) == 0) ? 1 : 0;
}

#ifdef CSH_MAIN
// A case in the file: int32 {B, size_x, size_y, n_beams, has_keep, has_cost, has_info, then ipar}, double {resolution, then dpar}, robot_pose, ranges (float), [keep],
// layer, layer_cell, [cost].  Its outputs in the other file: layer, layer_cell, [cost], [info].
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
        const size_t B = head[0], W = head[1], H = head[2], nb = head[3];
        std::vector<double> par, pose;
        std::vector<float> ranges;
        std::vector<int32_t> keep, cell, info(head[6] ? 4 * B : 0, -7);
        std::vector<uint8_t> layer, cost;
        if (!(rd(in, par, 13) && rd(in, pose, 3 * B) && rd(in, ranges, B * nb) && rd(in, keep, head[4] ? B : 0) && rd(in, layer, B * W * H) && rd(in, cell, 2 * B) &&
              rd(in, cost, head[5] ? B * W * H : 0))) { std::printf("case %d: short read\n", cases); return 2; }
        if (csh_scans((int)B, par.data() + 1, head.data() + 7, pose.data(), ranges.data(), (int)nb, head[4] ? keep.data() : nullptr, (int)W, (int)H, par[0], layer.data(),
                      cell.data(), head[5] ? cost.data() : nullptr, head[6] ? info.data() : nullptr) < 0) { std::printf("case %d: refused\n", cases); return 2; }
        if (!(wr(out, layer) && wr(out, cell) && wr(out, cost) && wr(out, info))) { std::printf("case %d: short write\n", cases); return 2; }
        ++cases;
    }
    std::fclose(in);
    std::fclose(out);
    std::printf("costmap_scans_host: %d cases\n", cases);
    return 0;
}
#endif
