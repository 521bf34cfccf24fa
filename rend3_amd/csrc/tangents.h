// tangents.h -- vertex tangents generated on the device for morphed meshes that ship without TANGENT (tangents.hip): argument block
// and launcher behind r3n_vertex_tangents (r3n.hip).
//
// Contract (DESIGN.md section 2 "Generated tangents", include/r3n.h; the definition is Mesh::calculate_tangents_for_buffers,
// rend3-types/src/lib.rs:784-837, zeroed = true, glam's scalar Vec3): for T = floor(index_count / 3) triangles t = (i0, i1, i2)
//     e1 = p[i1] - p[i0];  e2 = p[i2] - p[i0];  a = uv[i1] - uv[i0];  b = uv[i2] - uv[i0]
//     r = 1 / (a.x * b.y - a.y * b.x);  g_t = e1 * b.y - (e2 * a.y) * r                      (r multiplies the SECOND product only)
//     acc[v] = (+0, +0, +0);  for the triangles that name v, in ASCENDING triangle number, once per occurrence: acc[v] = fl(acc[v] + g_t)
//     d = (n.x * acc.x + n.y * acc.y) + n.z * acc.z;  q = acc - n * d                        (n = normal[v] as stored)
//     rcp = 1 / sqrt((q.x * q.x + q.y * q.y) + q.z * q.z);  out[v] = rcp finite and > 0 ? q * rcp : (+0, +0, +0)
// one rounding per operation (the unit is built with -ffp-contract=off).  Ascending triangle order per vertex is the order in which
// the reference's serial loop adds into tangents[v], so the gather gives the serial loop's words.  A triangle whose uv footprint is
// degenerate has r = +-inf, an inf or NaN term, and leaves every vertex it names at (+0, +0, +0): reproduced, not repaired.
//
// Adjacency: r3n_host_vertex_adjacency's words, as normals.h describes them.
#pragma once
#include "../../include/r3n.h"
#include "vertex_gather.h"

#define R3N_TANGENTS_WAVE_VERTICES 64u  // one thread per vertex

using TangentsArgs = vertex_gather::Args<r3n_tangents_input32>;  // 8 words each: one s_load_dwordx8

// enqueues the ONE launch on `stream`; returns the hipError_t of the launch
extern "C" int r3n_internal_vertex_tangents(const TangentsArgs *a, hipStream_t stream);
