// tests/hostsim/seed_bins.cpp -- TEST CODE, not part of the product: dev_fm.h compiled for the host on its own, for the unit test of the rule
// that bins the backward sweeps' tasks (tests/test_seed_bins_hostsim.py builds it into a small library of its own and calls the entry below).
#include <stdint.h>
#include "../../arachne_amd/csrc/arx_dev.h"
#include "../../arachne_amd/csrc/dev_fm.h"

// test entry: dev_fm.h seed_bwd_class -- the function the forward kernels' grant step calls -- for n list lengths
extern "C" void arx_test_seed_bwd_class(int n, const int32_t *len, int mid, int32_t *cls)
{
	for (int i = 0; i < n; ++i) cls[i] = arx::seed_bwd_class(len[i], mid);
}
