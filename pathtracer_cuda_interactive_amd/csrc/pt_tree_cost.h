// pt_tree_cost.h — the surface-area cost of a DNode array, summed on the device in a fixed order (pt_tree_cost.hip): the
// telemetry behind pt_scene_set_option "tree_cost" and the "rebuild_at_permille" policy.  Shared inside libpt_hip.so.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/pt_api.h"

namespace ptc {

// Cost of a tree = the sum, over every inner node below the root, of its box area in fp64:
//   e = (double)max - (double)min per axis,  a = 2.0 * ((ex * ey + ey * ez) + ez * ex),  operations as written, no contraction.
// A DNode carries its children's boxes, so this is one pass over the array adding the boxes of inner children (ref >= 0).
// (pt_host_tree_cost, include/pt_host.h, is the same expression over a node pool.)

// doubles of scratch a call needs for a tree of num_nodes DNodes (one partial per workgroup)
size_t partials_needed(int num_nodes);

// Enqueues both kernels on the default stream: partials_dev [partials_needed(num_nodes)] is scratch, *out_dev receives the
// cost.  Nothing is synchronised.  The order of every addition is fixed, so the result is the same bits on every run.
int tree_cost(const void* dnodes_dev, int num_nodes, double* partials_dev, double* out_dev);

}  // namespace ptc
