// pt_scene_transform.h — the record producer of pt_scene_transform (pt_scene_transform.hip): new primitive records from the
// rest records and one matrix per group.  Shared inside libpt_hip.so.
#pragma once
#include <stdint.h>

#include "../../include/pt_api.h"

namespace ptx {

// One launch on the default stream, nothing synchronised: record i of rest_prims_dev / rest_normals_dev (N DPrim / DNormals, 48 B
// each) under the entry of its group (pt_transform.h; group_dev [N], every id in [-1, num_groups) — the caller has checked them —,
// table_dev [num_groups] entries of 84 B) into out_prims_dev / out_normals_dev, which must not overlap the rest records.
// A group of -1 copies the record bit for bit.
int transform_records(const void* rest_prims_dev, const void* rest_normals_dev, const int32_t* group_dev, const float* table_dev,
                      int N, void* out_prims_dev, void* out_normals_dev);

}  // namespace ptx
