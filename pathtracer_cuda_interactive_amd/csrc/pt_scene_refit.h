// pt_scene_refit.h — device refit of a scene's two trees to new primitive records (pt_scene_refit.hip), the device half of
// pt_scene_update.  Shared inside libpt_hip.so.
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/pt_api.h"

namespace ptf {

// What a refit needs to know about one DNode array, made once from the array itself (topology never changes after
// pt_scene_create): 12 bytes per primitive.
//   parent_slot [num_nodes]  parent * 2 + side (side 1 = the node is its parent's RIGHT child), -1 for the root
//   leaf_slot   [N]          the same for every primitive's leaf
//   order       [num_nodes]  node ids sorted by depth; level_begin[d] .. level_begin[d + 1] are the nodes at depth d (root: 0)
struct Plan {
    void* arena = nullptr;               // one device allocation behind the four arrays
    int32_t* parent_slot = nullptr;
    int32_t* leaf_slot = nullptr;
    int32_t* order = nullptr;
    int32_t* level_begin = nullptr;      // [levels + 1], device copy of level_begin_host
    std::vector<int32_t> level_begin_host;
    int levels = 0;                      // depths 0 .. levels - 1 hold inner nodes
    int narrow_top = 0;                  // levels narrow_top .. 1 are done by the single-workgroup launch, deeper ones by a launch each
    bool whole_tree = false;             // leaves, every level and the octant tables fit that one launch
    bool built = false;
};

// dnodes_dev: num_nodes DNodes (64 B each) over N >= 2 primitives, root at index 0.
int plan_build(const void* dnodes_dev, int num_nodes, int N, Plan* out);
void plan_release(Plan* p);

// Leaf boxes of N staged DPrim records into boxes_dev [N][6] (min xyz, max xyz); *status_dev (zeroed by the caller) becomes
// non-zero when a value is not finite.  Sphere: c -/+ r; triangle: min(min(p0, p1), p2) / max per axis, min and max in the
// host pipeline's `a < b ? a : b` form (csrc/host/scene_build.cpp, vecmath.h).
int leaf_boxes(const void* prims_dev, int N, float* boxes_dev, unsigned int* status_dev);

// The leaf boxes a DNode array holds, back into the builders' layout (pt_scene_rebuild): one thread per node copies the boxes
// of its leaf children to boxes_dev [N][6].  num_nodes = N - 1 >= 1; a tree of that size over N primitives names each once
// (pt_scene_create checked), so every row is written.  Default stream, nothing synchronised.
int tree_leaf_boxes(const void* dnodes_dev, int num_nodes, int N, float* boxes_dev);

// Writes exact new boxes into one tree: leaf boxes into their parents' child slots, then every inner node's box = the union of
// its two child boxes into ITS parent's slot, levels deepest first; the 8 octant tables after that (dnodes_oct_dev, or null).
//   plan.whole_tree: ONE single-workgroup launch that computes the leaf boxes from prims_dev itself, checks them (a
//                    non-finite value: *status_dev set, nothing written) and does all of it; boxes_dev is not read.
//   otherwise:       boxes_dev must hold checked leaf boxes (leaf_boxes); one launch scatters them, one launch per level
//                    runs while levels are wide, one single-workgroup launch does the narrow top.
// Everything is enqueued on the default stream; nothing is synchronised here.
int refit_tree(const Plan& plan, void* dnodes_dev, void* dnodes_oct_dev, int num_nodes, const void* prims_dev,
               const float* boxes_dev, int N, unsigned int* status_dev);

}  // namespace ptf
