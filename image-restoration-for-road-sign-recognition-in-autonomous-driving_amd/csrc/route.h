// route.h -- which kernel one conv call runs: decided once per public call
// (conv_route, igemm.hip) from the descriptor, the call's RR_PATH snapshot and
// the call kind.  The partial-row count, the workspace size, the reported
// kernel name and the launch all read the same ConvRoute; the family
// launchers take the pick they are handed.  Internal; not part of the C ABI.
#pragma once
#include "common.h"
#include "stream1.h"
#include "stream3.h"

struct IgemmArgs;   // igemm_epi.h

// what the entry point is: rr_igemm, rr_igemm_bnbwd, rr_igemm_ex with an
// epilogue beyond ReLU, rr_igemm_pool without / with the window index,
// rr_igemm_dgrad_sc, rr_igemm_pre
enum ConvKind { CK_PLAIN, CK_BNBWD, CK_EX, CK_POOL, CK_POOL_IDX, CK_DGRAD_SC, CK_PRE };
enum ConvFamily { CF_NONE, CF_STREAM3, CF_STREAM1, CF_CONV3R, CF_HALO, CF_TILED };

// row-streaming 3x3 conv (stream3.hip): the kernel's flag set (< 0: not
// taken) and whether it walks the map in 32-wide column strips
struct S3Pick { int flags, strip; };
// wave-streaming 1x1 / convT GEMM (stream1.hip)
struct S1Plan { int mc, kb, nslice, G, key; };
// tap-reuse 3x3 conv (conv3r.hip): column block, per-wave channels, waves,
// halo buffers; sg > 0: row-segment tiles (any H x W)
struct R3Pick { int bc, nw, nwv, hb, sg; };

struct ConvRoute {
  int family;          // ConvFamily; CF_NONE: no kernel takes the call
  S3Pick s3;
  S1Plan s1;
  R3Pick r3;
  int halo_bc;         // LDS-halo igemm: column block
  int tile_bc, tile_bp;   // tiled igemm
  int rows;            // rows of the BN statistics / BN-backward partial slabs
  const char *name;    // the kernel instance (static string, never null)
};

ConvRoute conv_route(const rr_igemm_desc *d, const RrPath &p, int kind);

// ---- the families: one eligibility + pick function each (called by
// conv_route alone), the launcher and the name of a pick ----
S3Pick stream3_pick(const rr_igemm_desc *d, const RrPath &p, int kind);
int stream3_rows();
int stream3_launch(const rr_igemm_desc *d, S3Args a, S3Pick k, hipStream_t st);
// "stream3_kernel<64>" / "<32>" (whole rows), "<s32>" (column strips), with
// ",pool" / ",sc" for those call kinds
const char *stream3_name(const rr_igemm_desc *d, S3Pick k, int kind);

// workgroups per column slice (= rows of the stats partial slab) when the
// streaming kernel takes *d, else 0
int stream1_plan(const rr_igemm_desc *d, const RrPath &p, S1Plan *pl);
int stream1_launch(const rr_igemm_desc *d, const S1Plan &pl, S1Args a, hipStream_t st);
const char *stream1_name(const S1Plan &pl);

// the column block of *d's pick, 0 when the tap-reuse kernel does not take
// the descriptor (bf16 3x3, whole tiles)
int conv3r_bc(const rr_igemm_desc *d, const RrPath &p, R3Pick *k);
// rows of its partial slabs: one per wave row of a tile
int conv3r_rows(const rr_igemm_desc *d, R3Pick k);
// launch (a filled by igemm.hip's fill_args); returns an RR_* status
int conv3r_launch(const rr_igemm_desc *d, IgemmArgs &a, R3Pick k, hipStream_t st);
const char *conv3r_name(const rr_igemm_desc *d, R3Pick k);
