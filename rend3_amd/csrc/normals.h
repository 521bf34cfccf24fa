// normals.h -- vertex normals recomputed on the device for morphed meshes that ship without NORMAL (normals.hip): argument block
// and launcher behind r3n_vertex_normals (r3n.hip).
//
// Contract (DESIGN.md section 2 "Recomputed normals", include/r3n.h; the definition is Mesh::calculate_normals_for_buffers,
// rend3-types/src/lib.rs:662-704): for T = floor(index_count / 3) triangles t = (i0, i1, i2)
//     e1 = p[i1] - p[i0];  e2 = p[i2] - p[i0];  n_t = left_handed ? cross(e1, e2) : cross(e2, e1)
//     acc[v] = (+0, +0, +0);  for the triangles that name v, in ASCENDING triangle number, once per occurrence: acc[v] = fl(acc[v] + n_t)
//     rcp = 1 / sqrt((x * x + y * y) + z * z);  out[v] = rcp finite and > 0 ? acc[v] * rcp : (+0, +0, +0)
// one rounding per operation (the unit is built with -ffp-contract=off).  Ascending triangle order per vertex is the order in which
// the reference's serial loop adds into normals[v], so the gather below gives the serial loop's words.
//
// Adjacency (r3n_host_vertex_adjacency, host.cpp), vertex_count + 1 + 3 T words: rows[0 .. V], then the triangle numbers; row v =
// entries [rows[v], rows[v + 1]) of the list, the triangles naming v, ascending, one entry per occurrence.
#pragma once
#include "../../include/r3n.h"
#include "vertex_gather.h"

#define R3N_NORMALS_WAVE_VERTICES 64u  // one thread per vertex

using NormalsArgs = vertex_gather::Args<r3n_normals_input32>;  // 8 words each: one s_load_dwordx8

// enqueues the ONE launch on `stream`; returns the hipError_t of the launch
extern "C" int r3n_internal_vertex_normals(const NormalsArgs *a, hipStream_t stream);
