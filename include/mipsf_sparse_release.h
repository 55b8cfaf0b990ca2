/*
 * mipsf_sparse_release.h -- slots of the brick-sparse volume of mipsf_sparse.h given back: the bricks outside a box around the
 * camera, or the bricks mipsf_sparse_deintegrate left without an observed voxel, leave the pool (optionally into an archive the
 * caller keeps), the holes they leave are closed in place, and archived bricks come back later.  The volume's one structural
 * invariant holds before and after every call: THE SLOTS IN USE ARE 0 .. count-1, and a slot at or beyond `count` is all zero with
 * born = MIPSF_SPARSE_UNBORN, which is what mipsf_sparse_allocate expects of a slot it hands out.  A volume on which neither entry
 * point is called behaves byte for byte as without this header.  DESIGN.md 4.28; mipsfusion_amd/sparse_tsdf.py (release, restore,
 * BrickArchive, sparse_tsdf_odometry(keep_radius=...)).
 *
 * Same conventions as mipsf_sparse.h: int return code, message through mipsf_last_error(), one argument block with `struct_size`
 * first, DEVICE pointers, everything enqueued on `stream`, kernels only (a call replays from a captured graph), no allocation, no
 * synchronisation, no host round trip.  No floating-point atomic: the marks are an integer atomic minimum, the counts integer sums.
 * Nothing here computes a floating-point value: the predicates COMPARE stored float64 and fp32 words and the rest copies words bit
 * for bit, so there is no last bit that could decide anything and a restatement on the host (tests/sparse_release_cpu.py) gives
 * the same words.  The same call gives the same bytes.
 */
#ifndef MIPSF_SPARSE_RELEASE_H
#define MIPSF_SPARSE_RELEASE_H

#include <stdint.h>

#include "mipsf_sparse.h"
#include "mipsf_sparse_remove.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mipsf_sparse_release_args.flags */
#define MIPSF_SPARSE_RELEASE_OUTSIDE 1u          /* predicate: the brick's voxel-centre box lies outside `box`                     */
#define MIPSF_SPARSE_RELEASE_EMPTY 2u            /* predicate: no word of the slot's weight is > 0                                 */
#define MIPSF_SPARSE_RELEASE_ARCHIVE 4u          /* the released slots are written to the archive, at most archive_capacity of them */

#define MIPSF_SPARSE_RESTORE_SCRATCH_WORDS 16u   /* uint32 words of mipsf_sparse_restore_args.scratch                              */

/* An archive is the caller's, on the device, `cap` entries:
 *   arch_brick  int32  [cap]            the brick an entry held
 *   arch_born   uint32 [cap]            its born (mipsf_sparse_remove.h); there exactly when the volume has a history (`born`)
 *   arch_tsdf, arch_weight fp32 [cap,8,8,16];  arch_color fp32 [cap,8,8,16,3], there exactly when the volume has colour
 * all the words of a slot, those outside the grid too, bit for bit. */

typedef struct mipsf_sparse_release_record {
    uint64_t candidates;                /* slots in use for which an enabled predicate holds                                    */
    uint64_t released;                  /* of those, slots given back                                                           */
    uint64_t released_outside;          /* released slots for which OUTSIDE was enabled and held                                */
    uint64_t released_empty;            /* released slots for which EMPTY was enabled and held (a slot may count in both)       */
    uint64_t deferred;                  /* candidates the archive had no room for: they stay in the volume                      */
    uint64_t moved;                     /* slots moved to close the holes                                                       */
    uint64_t in_use;                    /* slots in use after the call                                                          */
} mipsf_sparse_release_record;

/* uint32 words of the `scratch` of mipsf_sparse_release for a pool of `capacity` slots; 0: capacity is 0 or above
 * MIPSF_SPARSE_MAX_CAPACITY */
uint64_t mipsf_sparse_release_scratch_words(uint32_t capacity);

/* mipsf_sparse_release.  With n = min(count, capacity), per slot s < n and brick b = slot_brick[s] = (bx, by, bz), B = (8, 8, 16):
 *
 * Predicates.
 *   OUTSIDE  blo[a] = ticks[a][B_a*b_a],  bhi[a] = ticks[a][min(B_a*b_a + B_a - 1, D_a - 1)]   (read, nothing is computed)
 *            with box = lo[3], hi[3] in world metres:  outside = for some axis a,  bhi[a] < lo[a] || blo[a] > hi[a]
 *            compared as float64.  A NaN in the box fails every comparison and releases nothing.
 *   EMPTY    none of the 1024 words of weight[s] is > 0   (a NaN weight is not > 0)
 *   r[s] = 1 when an enabled predicate holds ("candidate"), else 0;  r[s] = 0 for s >= n.
 *
 * Archive cap.  cap = archive_capacity with MIPSF_SPARSE_RELEASE_ARCHIVE, unbounded without.  R(s) = sum of r[t], t < s (one
 * prefix sum over tiles of MIPSF_SPARSE_SCAN_TILE slots, as in mipsf_sparse_allocate).  Slot s is RELEASED when r[s] && R(s) < cap:
 * the first cap candidates in ascending slot order; the others stay (`deferred`).  F(s) = min(R(s), cap) is the count of released
 * slots before s.
 *
 * Archive.  The k-th released slot in ascending slot order (F(s) = k) writes entry k: arch_brick[k] = slot_brick[s],
 * arch_born[k] = born[s], and the words of tsdf, weight and colour.  Entries at or beyond `released` are not touched.
 *
 * Closing the holes, after the archive is written.  n' = n - released.  The released slots below n' are the holes; the slots
 * n' <= s < n that are not released are the tail survivors; there are as many of the one as of the other (`moved`).  The j-th tail
 * survivor in ascending slot order moves into the j-th hole in ascending slot order: all words of tsdf, weight and colour,
 * slot_brick, born, and table[its brick] = the hole.  Sources (>= n') and destinations (< n') are disjoint.  Every released brick
 * gets table = -1.  Every slot n' <= s < n is then left all zero (tsdf, weight, colour) with born[s] = MIPSF_SPARSE_UNBORN.
 * count = n' is written by the last launch, after every kernel that reads the old value.  Slots below n' that are not holes are not
 * touched; birth is not touched; nothing is written at or beyond slot n.
 *
 * record: written whole by the last launch.
 * Refused on the host, with nothing launched: what mipsf_sparse_allocate refuses of the volume; flags other than the three above,
 * or neither predicate; OUTSIDE without a box; with ARCHIVE and archive_capacity > 0 a null arch_brick, arch_tsdf or arch_weight,
 * a null arch_color while vol.color is there, a null arch_born while born is there; a null scratch or one not aligned to 8 bytes;
 * a null record. */
typedef struct mipsf_sparse_release_args {
    uint32_t struct_size;
    uint32_t flags;
    uint32_t archive_capacity;          /* entries of the archive; read with MIPSF_SPARSE_RELEASE_ARCHIVE only                  */
    uint32_t reserved;
    mipsf_sparse_volume vol;
    uint32_t* born;                     /* [capacity] or null: the history of the volume                                        */
    const double* box;                  /* [6] lo[3], hi[3]; with OUTSIDE                                                       */
    int32_t* arch_brick;                /* [archive_capacity]                                                                   */
    uint32_t* arch_born;                /* [archive_capacity] or null                                                           */
    float* arch_tsdf;                   /* [archive_capacity,8,8,16]                                                            */
    float* arch_weight;                 /* [archive_capacity,8,8,16]                                                            */
    float* arch_color;                  /* [archive_capacity,8,8,16,3] or null                                                  */
    uint32_t* scratch;                  /* [mipsf_sparse_release_scratch_words(capacity)]                                       */
    mipsf_sparse_release_record* record;
} mipsf_sparse_release_args;

int mipsf_sparse_release(const mipsf_sparse_release_args* a, void* stream);

typedef struct mipsf_sparse_restore_record {
    uint64_t listed;                    /* m                                                                                    */
    uint64_t invalid;                   /* entries whose brick is not a brick of the grid                                       */
    uint64_t duplicates;                /* valid entries that lost their brick to an entry with a lower index                    */
    uint64_t occupied;                  /* bricks listed that have a slot already: they keep their words                        */
    uint64_t restored;                  /* bricks that got a slot and their entry's words                                       */
    uint64_t dropped;                   /* bricks that got none: the pool was full                                              */
    uint64_t in_use;                    /* slots in use after the call                                                          */
} mipsf_sparse_restore_record;

/* mipsf_sparse_restore: m entries of an archive come back.  mark (uint32 [BX,BY,BZ]) and scan are the scratch of
 * mipsf_sparse_allocate.  mark is set to 0xffffffff; every entry k with 0 <= arch_brick[k] < bricks does
 * mark[brick] = min(mark[brick], k), so the lowest entry wins a brick listed twice whatever the order of work.  The steps of
 * mipsf_sparse_allocate (its own kernels) then give the marked bricks without a slot the slots count, count + 1, .. in ascending
 * brick index, table and slot_brick written and birth[slot] = k, the pool's end as there (`dropped`); birth of the slots in use
 * before is 0.  One workgroup per new slot copies the words of entry birth[slot] into it, and born[slot] = arch_born[birth[slot]].
 * A marked brick that has a slot already keeps its words (`occupied`).  m = 0 is a no-op with a zero record: only the record is written.
 * Refused on the host, with nothing launched: what mipsf_sparse_allocate refuses of the volume; m above MIPSF_SPARSE_MAX_CAPACITY;
 * with m > 0 a null arch_brick, arch_tsdf or arch_weight, arch_color and vol.color not both there or both null, arch_born and
 * born likewise; a null mark, scan, scratch or record. */
typedef struct mipsf_sparse_restore_args {
    uint32_t struct_size;
    uint32_t m;
    mipsf_sparse_volume vol;
    uint32_t* born;                     /* [capacity] or null                                                                   */
    const int32_t* arch_brick;          /* [m]                                                                                  */
    const uint32_t* arch_born;          /* [m] or null                                                                          */
    const float* arch_tsdf;             /* [m,8,8,16]                                                                           */
    const float* arch_weight;           /* [m,8,8,16]                                                                           */
    const float* arch_color;            /* [m,8,8,16,3] or null                                                                 */
    uint32_t* mark;                     /* [BX,BY,BZ]                                                                           */
    uint32_t* scan;                     /* [mipsf_sparse_scan_words(X, Y, Z)]                                                   */
    uint32_t* scratch;                  /* [MIPSF_SPARSE_RESTORE_SCRATCH_WORDS], aligned to 8 bytes                             */
    mipsf_sparse_restore_record* record;
} mipsf_sparse_restore_args;

int mipsf_sparse_restore(const mipsf_sparse_restore_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIPSF_SPARSE_RELEASE_H */
