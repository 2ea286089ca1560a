// gicp.hpp -- what reg.hip (which owns the registration handle and the 1-NN passes) calls of gicp.hip.
#pragma once
#include "p2l.hpp"  // Call, Ctx, the workspace: the batch is the point-to-plane refinement's

namespace gloc {
namespace gicp {

int check_params(const gloc_gicp_params* prm);
// As p2l::run, with the sources' normals (x.srcs[c].nrm, the order of its pts; zero = none) beside the targets'.
int run(const p2l::Ctx& x, const gn6::Target* tgts, const gn6::Call& c, const gloc_gicp_params* prm);

}  // namespace gicp
}  // namespace gloc
