// gicp.hpp -- what reg.hip (which owns the registration handle and the 1-NN passes) calls of gicp.hip.
#pragma once
#include "p2l.hpp"  // Ctx, TargetView, the workspace: the batch is the point-to-plane refinement's

namespace gloc {
namespace gicp {

int check_params(const gloc_gicp_params* prm);
// As p2l::run, with the sources' normals (x.srcs[c].nrm, the order of its pts; zero = none) beside the targets'.
int run(const p2l::Ctx& x, const p2l::TargetView* tgts, const float* init_T, const gloc_gicp_params* prm,
        float* out_T, float* out_rmse, uint32_t* out_iters, int* out_status, double* out_H36, double* out_g6, double* out_sum,
        uint64_t* out_count, const p2l::RobustArgs& rb = p2l::RobustArgs());

}  // namespace gicp
}  // namespace gloc
