// gbp_transport.hpp — the transports of the sharded exchange by name.  The values are those of the public
// gbp_comm_init(ctx, region, transport) argument (include/gbp_mi355x_multi.h).  No HIP in here: the CLIs, plain C++ on top of the
// C-ABI, include it next to the library (gbp_comm.hpp).
#pragma once

namespace gbp {

enum class Transport : int {
  Auto = 0,        // RCCL when every rank sits on its own GPU, host-staged otherwise
  Rccl = 1,
  HostStaged = 2,
  P2p = 3,         // direct peer memory; never chosen by Auto
  P2pSlices = 4,   // the same, cameras reduced in slices; never chosen by Auto
};

}  // namespace gbp
