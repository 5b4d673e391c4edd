// tests only: the host build of mpc_local_planner_amd/csrc/mpc_costmap_window.hpp (the per-instance rule of mpc_costmap_window*) behind a C entry point, in the
// layouts of include/mpc_costmap_window.h.  No GPU calls.  With -DCWH_MAIN: a stand-alone program that reads cases from a file written by tests/_window_cases.py
// (write_cases), runs them through the same entry point and writes the outputs to another file (the sanitizer build of tests/test_costmap_window_host.py).
#include "../../mpc_local_planner_amd/csrc/mpc_costmap_window.hpp"

#include <cstdio>
#include <vector>

// B instances through cw_instance, the table by cw_table.  dpar: {map_origin x, y, map_resolution, lattice_anchor x, y, inscribed_radius, inflation_radius,
// cost_scaling_factor}; ipar: {map_size_x, map_size_y, outside_value, inflate_unknown}; info [B][4] and d2 [B][size_y][size_x] nullable.  Returns rule 3's r, -1 when
// it is above the limit (nothing is written then).
extern "C" int cwh_window(int B, const uint8_t* map, const double* dpar, const int32_t* ipar, const double* robot_pose, int size_x, int size_y, double resolution,
                          uint8_t* cost, double* origin, int32_t* info, int32_t* d2) {
    const int r = mpc::cw_cell_radius(dpar[6], resolution);
    if (r < 0) return -1;
    const mpc::WindowParams p = {dpar[0], dpar[1], dpar[2], dpar[3], dpar[4], resolution, ipar[0], ipar[1], ipar[2], ipar[3] ? 1 : 0, r};
    std::vector<uint8_t> table((size_t)r * r + 1);
    mpc::cw_table(resolution, dpar[5], dpar[7], r, table.data());
    const size_t cells = (size_t)size_x * size_y;
    for (int b = 0; b < B; ++b)
        mpc::cw_instance(p, table.data(), map, robot_pose + 3 * (size_t)b, size_x, size_y, cost + b * cells, origin + 2 * (size_t)b, info ? info + 4 * (size_t)b : nullptr,
                         d2 ? d2 + b * cells : nullptr);
    return r;
}

// rule 4 alone: table[0 .. r * r]
extern "C" void cwh_table(double resolution, double inscribed_radius, double cost_scaling_factor, int r, uint8_t* table) {
    mpc::cw_table(resolution, inscribed_radius, cost_scaling_factor, r, table);
}

// the kernel's tile and the largest radius, for the cases that have to span three tiles
extern "C" int cwh_tile_x() { return mpc::kCwTileX; }
extern "C" int cwh_tile_y() { return mpc::kCwTileY; }
extern "C" int cwh_max_r() { return mpc::kCwMaxR; }

#ifdef CWH_MAIN
// A case in the file: int32 {B, size_x, size_y, map_size_x, map_size_y, outside_value, inflate_unknown, has_info}, double {resolution, then dpar}, the map, robot_pose.
// Its outputs in the other file: cost, origin, [info].
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
    while (rd(in, head, 8)) {
        const size_t B = head[0], W = head[1], H = head[2];
        std::vector<double> par, pose, origin(2 * B, -1.0);
        std::vector<uint8_t> map, cost(B * W * H, 0xA5);
        std::vector<int32_t> info(head[7] ? 4 * B : 0, -7);
        if (!(rd(in, par, 9) && rd(in, map, (size_t)head[3] * head[4]) && rd(in, pose, 3 * B))) { std::printf("case %d: short read\n", cases); return 2; }
        if (cwh_window((int)B, map.data(), par.data() + 1, head.data() + 3, pose.data(), (int)W, (int)H, par[0], cost.data(), origin.data(), head[7] ? info.data() : nullptr, nullptr) < 0) {
            std::printf("case %d: refused\n", cases); return 2; }
        if (!(wr(out, cost) && wr(out, origin) && wr(out, info))) { std::printf("case %d: short write\n", cases); return 2; }
        ++cases;
    }
    std::fclose(in);
    std::fclose(out);
    std::printf("costmap_window_host: %d cases\n", cases);
    return 0;
}
#endif
