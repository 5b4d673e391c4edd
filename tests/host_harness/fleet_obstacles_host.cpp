// tests only: the host build of mpc_local_planner_amd/csrc/mpc_fleet_obstacles.hpp (the per-instance rules of mpc_obstacles_from_pool* and mpc_fleet_pool*) behind C entry
// points, in the layouts of include/mpc_fleet.h.  No GPU calls.  With -DFOB_MAIN: a stand-alone program that reads cases from a file written by
// tests/_fleet_cases.py (write_cases), runs them through the same entry points and writes the outputs to another file (the sanitizer build of
// tests/test_fleet_obstacles_host.py).
#include "../../mpc_local_planner_amd/csrc/mpc_fleet_obstacles.hpp"

#include <cstdio>
#include <vector>

// B instances through fo_instance; every pointer as in mpc_obstacles_from_pool (radius / velocity / self_index / dropped / n_taken nullable)
extern "C" void fob_select(int B, int P, const int32_t* pool_n_vertices, const double* pool_vertices, const double* pool_radius, const double* pool_velocity, int V, int O,
                           const double* robot_pose, const int32_t* self_index, double reach, double min_speed, int append, int32_t* n_obstacles, int32_t* n_vertices,
                           double* vertices, double* radius, double* velocity, int32_t* dropped, int32_t* n_taken) {
    const mpc::FleetPool pool = {P, pool_n_vertices, pool_vertices, pool_radius, pool_velocity};
    const mpc::FleetParams prm = {reach, min_speed, append};
    for (int b = 0; b < B; ++b) {
        const mpc::FleetContainer c = {n_vertices + (size_t)b * O, vertices + (size_t)b * O * V * 2, radius ? radius + (size_t)b * O : nullptr, velocity ? velocity + (size_t)b * O * 2 : nullptr};
        mpc::fo_instance(pool, V, O, robot_pose[3 * b], robot_pose[3 * b + 1], self_index ? self_index[b] : -1, prm, n_obstacles + b, c, dropped ? dropped + b : nullptr,
                         n_taken ? n_taken + b : nullptr);
    }
}

// B robots through fp_instance; every pointer as in mpc_fleet_pool (x: [B][n_stride][3])
extern "C" void fob_pool(int B, const double* robot_pose, const double* x, int n_stride, const double* dt, const int32_t* status, double robot_radius, const double* radius, int V,
                         int pool_offset, int32_t* pool_n_vertices, double* pool_vertices, double* pool_radius, double* pool_velocity) {
    for (int b = 0; b < B; ++b)
        mpc::fp_instance(robot_pose + 3 * b, x ? x + (size_t)b * n_stride * 3 : nullptr, x ? dt[b] : 0.0, status ? status[b] == 0 : true, radius ? radius[b] : robot_radius, V,
                         pool_offset + b, pool_n_vertices, pool_vertices, pool_radius, pool_velocity);
}

#ifdef FOB_MAIN
// A case in the file: int32 {B, P, V, O, has_pool_radius, has_pool_velocity, has_self, append, has_radius, has_velocity}, double {reach, min_speed}, then the arrays in the
// order of fob_select's parameters (absent ones left out).  Its outputs in the other file: n_obstacles, n_vertices, vertices, [radius], [velocity], dropped, n_taken.
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
    while (rd(in, head, 10)) {
        const size_t B = head[0], P = head[1], V = head[2], O = head[3];
        std::vector<double> par, pv, pr, pvel, pose, vt, rad, vel;
        std::vector<int32_t> pnv, self, no, nv, dropped(B, -1), taken(B, -1);
        bool ok = rd(in, par, 2) && rd(in, pnv, P) && rd(in, pv, P * V * 2) && rd(in, pr, head[4] ? P : 0) && rd(in, pvel, head[5] ? 2 * P : 0) && rd(in, pose, 3 * B) &&
                  rd(in, self, head[6] ? B : 0) && rd(in, no, B) && rd(in, nv, B * O) && rd(in, vt, B * O * V * 2) && rd(in, rad, head[8] ? B * O : 0) && rd(in, vel, head[9] ? B * O * 2 : 0);
        if (!ok) { std::printf("case %d: short read\n", cases); return 2; }
        fob_select((int)B, (int)P, pnv.data(), pv.data(), head[4] ? pr.data() : nullptr, head[5] ? pvel.data() : nullptr, (int)V, (int)O, pose.data(), head[6] ? self.data() : nullptr, par[0], par[1],
                   head[7], no.data(), nv.data(), vt.data(), head[8] ? rad.data() : nullptr, head[9] ? vel.data() : nullptr, dropped.data(), taken.data());
        if (!(wr(out, no) && wr(out, nv) && wr(out, vt) && wr(out, rad) && wr(out, vel) && wr(out, dropped) && wr(out, taken))) { std::printf("case %d: short write\n", cases); return 2; }
        ++cases;
    }
    std::fclose(in);
    std::fclose(out);
    std::printf("fleet_obstacles_host: %d cases\n", cases);
    return 0;
}
#endif
