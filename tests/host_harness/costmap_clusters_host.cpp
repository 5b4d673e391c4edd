// tests only: the host build of mpc_local_planner_amd/csrc/mpc_costmap_clusters.hpp (the per-instance rule of mpc_costmap_to_polygons*) behind a C entry point, in the
// layouts of include/mpc_costmap_clusters.h.  No GPU calls.  With -DCCH_MAIN: a stand-alone program that reads cases from a file written by tests/_cluster_cases.py
// (write_cases), runs them through the same entry point and writes the outputs to another file (the sanitizer build of tests/test_costmap_clusters_host.py).
#include "../../mpc_local_planner_amd/csrc/mpc_costmap_clusters.hpp"

#include <vector>

// B instances through cc_instance; every pointer as in mpc_costmap_to_polygons (radius / velocity / dropped / info nullable)
extern "C" void cch_polygons(int B, const uint8_t* cost, int size_x, int size_y, double resolution, const double* origin, const double* robot_pose, double behind_robot_dist,
                             int link_dist_sq, int V, int O, int32_t* n_obstacles, int32_t* n_vertices, double* vertices, double* radius, double* velocity, int32_t* dropped,
                             int32_t* info) {
    const mpc::ClusterParams prm = {behind_robot_dist, link_dist_sq};
    const mpc::CcBatch a = {cost, origin, robot_pose, size_x, size_y, resolution, O, V, nullptr, n_obstacles, n_vertices, vertices, radius, velocity, dropped, info};
    std::vector<int32_t> lab((size_t)size_x * size_y);
    for (int b = 0; b < B; ++b) {
        mpc::CcMap m;
        mpc::CcContainer c;
        mpc::cc_view(a, b, m, c);
        mpc::cc_instance(m, prm, V, O, lab.data(), n_obstacles + b, c, dropped ? dropped + b : nullptr, info ? info + 4 * b : nullptr);
    }
}

#ifdef CCH_MAIN
#include "costmap_case_file.hpp"
// the header words: {B, size_x, size_y, V, O, link_dist_sq, has_radius, has_velocity}
int main(int argc, char** argv) {
    return run_case_file<8, 6>(argc, argv, "costmap_clusters_host", [](const int32_t* head, double resolution, double behind_robot_dist, const CaseArrays& x) {
        cch_polygons(head[0], x.cost, head[1], head[2], resolution, x.origin, x.pose, behind_robot_dist, head[5], head[3], head[4], x.n_obstacles, x.n_vertices, x.vertices,
                     x.radius, x.velocity, x.dropped, x.info);
    });
}
#endif
