/*
 * poseidon_mi355x.h -- C ABI of the MI355X-native batched Poseidon permutation / duplex sponge.
 *
 * Drop-in boundary for the Poseidon hot path of arkworks-rs/sponge (ark-sponge).  The reference has
 * no FFI seam of its own (src/lib.rs:10 forbids unsafe); the seam is its generic trait surface.  Each
 * entry point below names the reference interface it replaces.  The Rust-side binding a maintainer
 * adds is shown in INTEGRATION.md.
 *
 * Element representation (everywhere in this ABI): a field element is 4 little-endian uint64_t limbs
 * holding the fully reduced Montgomery residue  x * 2^256 mod p  -- byte-identical to ark-ff's
 * Fp<MontBackend<_,4>,4>, so a Rust &[Fr] / Vec<Fr> is passed as-is (src/poseidon/mod.rs:57 `state`).
 * "Bit-exact" means limb-for-limb equality of these residues.  Inputs must be fully reduced, as ark-ff keeps them:
 * config constants are checked, batch data is not, and the result for an unreduced state or message element is
 * unspecified (the permutation kernels happen to process it modulo p; the absorb driver adds elements into the state
 * as 256-bit residues with ONE conditional subtraction, which is exact only for reduced operands).
 *
 * State order inside one sponge state is the reference's: capacity elements first, then the rate
 * elements (src/poseidon/mod.rs:128,143,159).
 *
 * All functions return PMX_OK (0) or a negative pmx_status; pmx_last_error() gives the message of the
 * calling thread's last failure.  Nothing throws or aborts across the boundary (the reference panics:
 * src/poseidon/mod.rs:196-203): every entry point that allocates, locks or spawns runs inside a catch-all that turns
 * std::bad_alloc / std::system_error / anything else into PMX_ERR_HOST.  There is NO CPU fallback: without a usable HIP device every data-path
 * call fails with PMX_ERR_HIP.
 *
 * Threading: the host-buffer entry points of one pmx_ctx serialise on a lock inside the context (they share its
 * staging buffers and streams); the *_dev entry points only enqueue on the caller's stream and may be called
 * concurrently (the absorb / squeeze ones take a short lock inside the context while they enqueue).  Distinct contexts are independent.  Every call runs with its context's device current and restores
 * the calling thread's current HIP device before it returns; a `stream` argument must belong to the context's device.
 *
 * Graph capture (*_dev entry points): each entry below says whether it may be captured into a hipGraph.  Those that may only launch
 * kernels and device-to-device copies on the caller's stream: they allocate nothing, synchronise nothing, ask the stream nothing and keep
 * no host copy of the data, so a captured call records all its work and nothing else, executes nothing while it is captured, needs no
 * earlier call to warm anything up (the captured launch may be the first launch of its kernel in the process) and on replay works on
 * whatever the buffers then hold (tests/test_gpu_streams.py).  The pass-form drivers, the variable-length entries and squeeze bytes /
 * bits must NOT be captured: their scratch comes from a per-stream pool of the context that may call hipMalloc.  The pmx_mgpu_*_dev
 * entries enqueue on the group's own streams and are not meant for capture.
 *
 * Alignment of device pointers (*_dev entry points): every array of field elements - states, messages, digests, nodes, leaves,
 * paths, the root, d_work - must be 16-byte aligned (PMX_ERR_ARG "device pointers must be 16-byte aligned" otherwise, nothing
 * launched).  Every other array needs the natural alignment of its element type and no more: mode words (d_mode_tag, d_mode_index:
 * uint32_t) 4 bytes, d_offsets and d_indices (uint64_t) 8 bytes, d_ok (uint8_t) any address.  Nothing beyond these is assumed: buffers
 * carved out of one allocation at base + 16 k are as good as allocations of their own, and a call writes nothing outside the arrays
 * it is documented to write (tests/test_gpu_footprint.py).  The host-buffer entry points accept any host pointer.
 *
 * Refused calls (host-buffer entry points): every argument is validated before anything is staged, so a call that returns PMX_ERR_ARG
 * has launched nothing and has written no byte of any of the caller's arrays (tests/test_gpu_host_footprint.py).
 */
#ifndef POSEIDON_MI355X_H
#define POSEIDON_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 3: PMX_ERR_HOST, pmx_merkle_verify_paths_dev, indices >= 2^depth fail verification, pmx_ctx_engine_info,
 *    pmx_merkle_2to1_forest[_dev]; the test hooks left this header (poseidon_mi355x_testing.h).
 * 4: the benchmark diagnostics (pmx_diag_*) left the library for libposeidon_mi355x_diag.so (poseidon_mi355x_diag.h); the host-buffer
 *    absorb / squeeze take any length (they cut a call longer than 65536 rates into pieces).
 * 5: pmx_mgpu_gather_dev (the result to one rank), pmx_mgpu_permute_gather_dev (the last step and its gather, overlapped). */
#define PMX_ABI_VERSION 5
#define PMX_LIMBS 4        /* uint64_t limbs per field element */
#define PMX_MAX_WIDTH 16   /* largest rate+capacity accepted (reference default table uses 3..9) */

typedef enum pmx_status {
    PMX_OK = 0,
    PMX_ERR_CONFIG = -1,      /* violates the asserts of PoseidonConfig::new (src/poseidon/mod.rs:196-203) or a limit of this build */
    PMX_ERR_ARG = -2,         /* null pointer / bad size / bad mode word */
    PMX_ERR_HIP = -3,         /* HIP runtime failure or no device */
    PMX_ERR_UNSUPPORTED = -4, /* width without a compiled kernel */
    PMX_ERR_RCCL = -5,        /* RCCL failure in a device group (pmx_mgpu_*) */
    PMX_ERR_HOST = -6         /* host resource failure inside the library: out of memory, a lock or a thread could not be made */
} pmx_status;

/* DuplexSpongeMode (src/lib.rs:198-210) as two words per sponge: tag + index. */
#define PMX_MODE_ABSORBING 0u /* index = next_absorb_index  in [0, rate] */
#define PMX_MODE_SQUEEZING 1u /* index = next_squeeze_index in [0, rate] */

/*
 * PoseidonConfig<F> (src/poseidon/mod.rs:23-42) plus the prime.  ark / mds are borrowed for the
 * duration of pmx_ctx_create only.
 */
typedef struct pmx_config {
    uint32_t full_rounds;            /* PoseidonConfig::full_rounds (RF/2 before the partial rounds, RF - RF/2 after, mod.rs:96-116) */
    uint32_t partial_rounds;         /* PoseidonConfig::partial_rounds */
    uint64_t alpha;                  /* PoseidonConfig::alpha, S-box exponent */
    uint32_t rate;                   /* PoseidonConfig::rate */
    uint32_t capacity;               /* PoseidonConfig::capacity */
    uint64_t modulus[PMX_LIMBS];     /* p, canonical little-endian limbs (odd, < 2^256) */
    const uint64_t *ark;             /* [full_rounds+partial_rounds][rate+capacity][4]  ark[round][i] */
    const uint64_t *mds;             /* [rate+capacity][rate+capacity][4]               mds[i][j], row-major */
} pmx_config;

typedef struct pmx_ctx pmx_ctx;

/* ---- library / error ------------------------------------------------------------------------- */
int pmx_abi_version(void);
const char *pmx_last_error(void);
/* Number of HIP devices visible (0 when none; never fails). */
int pmx_device_count(void);

/* ---- pinned host memory (optional) --------------------------------------------------------------
 * The host-buffer entry points below accept any host pointer.  When a buffer is page-locked (allocated here, or
 * registered by the caller with hipHostRegister) they switch from the runtime's pageable staging to a chunked
 * H2D / kernel / D2H pipeline on three streams: 2^20 states round-trip in 2.5 ms instead of 9-15 ms. */
int pmx_host_alloc(void **ptr, size_t bytes);
int pmx_host_free(void *ptr);

/* ---- device memory for the *_dev entry points (optional) ------------------------------------------
 * A caller that already manages HIP memory passes its own device pointers and streams.  One that does not (a Rust
 * crate without HIP bindings) gets what it needs here: allocation on a device, copies ordered on a stream (NULL = the
 * device's default stream; copies from / to pageable host memory complete before the call returns, page-locked ones
 * are asynchronous), and a stream wait. */
int pmx_device_alloc(int device, void **d_ptr, size_t bytes);
int pmx_device_free(int device, void *d_ptr);
int pmx_device_upload(int device, void *d_dst, const void *h_src, size_t bytes, void *stream);
int pmx_device_download(int device, void *h_dst, const void *d_src, size_t bytes, void *stream);
int pmx_stream_synchronize(int device, void *stream);

/* ---- parameters (host only) -------------------------------------------------------------------
 * find_poseidon_ark_and_mds (src/poseidon/traits.rs:105-146) with PoseidonGrainLFSR
 * (src/poseidon/grain_lfsr.rs:15-189): width = rate+1.  Writes Montgomery residues:
 * ark_out [(full_rounds+partial_rounds)*(rate+1)*4], mds_out [(rate+1)*(rate+1)*4]. */
int pmx_find_poseidon_ark_and_mds(const uint64_t modulus[PMX_LIMBS], uint64_t prime_bits, uint32_t rate,
                                  uint32_t full_rounds, uint32_t partial_rounds, uint32_t skip_matrices,
                                  uint64_t *ark_out, uint64_t *mds_out);

/* Montgomery constants of a modulus: inv = -p^-1 mod 2^64, r = 2^256 mod p, r2 = 2^512 mod p. */
int pmx_mont_constants(const uint64_t modulus[PMX_LIMBS], uint64_t *inv, uint64_t r[PMX_LIMBS],
                       uint64_t r2[PMX_LIMBS]);
/* canonical -> Montgomery / Montgomery -> canonical, in place over n elements (ark-ff from_bigint / into_bigint). */
int pmx_to_mont(const uint64_t modulus[PMX_LIMBS], uint64_t *elems, size_t n);
int pmx_from_mont(const uint64_t modulus[PMX_LIMBS], uint64_t *elems, size_t n);

/* ---- context ----------------------------------------------------------------------------------
 * CryptographicSponge::new's parameter clone (src/poseidon/mod.rs:219-230) happens once here: the
 * config is validated like PoseidonConfig::new (src/poseidon/mod.rs:187-213) and its constants are
 * uploaded to `device`.  */
int pmx_ctx_create(const pmx_config *cfg, int device, pmx_ctx **out);
int pmx_ctx_destroy(pmx_ctx *ctx);
/* The same context from a process-wide cache keyed by (config contents, device), reference-counted: what a binding's
 * CryptographicSponge::new should call, so that a sponge per transcript (the reference's usage, mod.rs:219-230 clones
 * ~4 KB of parameters per sponge) costs a hash of the constants, not a table derivation + upload.  Contexts whose
 * count drops to zero stay resident (a few, oldest evicted first); pmx_ctx_cache_clear frees the idle ones. */
int pmx_ctx_acquire(const pmx_config *cfg, int device, pmx_ctx **out);
int pmx_ctx_release(pmx_ctx *ctx);
int pmx_ctx_cache_clear(void);
/* width t = rate + capacity of the context's config */
int pmx_ctx_width(const pmx_ctx *ctx);

/* ---- which engine a call runs on --------------------------------------------------------------------
 * The launchers pick a kernel family by width, exponent, schedule, modulus and batch size.  This
 * reports the choice for one call, through the launchers' own conditions, so that a benchmark's instruction accounting
 * cannot drift from the kernels: op = one of PMX_OP_*, n = units of the call (states, rows, compressions of one tree
 * level, sponges), len = in_len / out_len of an absorb / squeeze call, the arity of a PMX_OP_COMPRESS level when it is 3 or more (the
 * engine does not depend on it; ignored otherwise).  Host only; nothing is
 * launched.  The reference has no counterpart (one code path, src/poseidon/mod.rs:95-118). */
#define PMX_OP_PERMUTE 0
#define PMX_OP_HASH 1
#define PMX_OP_COMPRESS 2
#define PMX_OP_ABSORB 3
#define PMX_OP_SQUEEZE 4
#define PMX_OP_GRIND 5     /* one chunk of n candidates of pmx_sponge_grind */
typedef struct pmx_engine_info {
    char engine[64];     /* e.g. "QuadEngine<5>", "HybridEngine<9,5,mfma,windows of 9>", "... x passes", "LdsEngine<5>" */
    int width;           /* t */
    int threads;         /* per workgroup */
    int waves_per_simd;  /* the kernel's launch bound (what its register allocation is held to) */
    int lds_bytes;       /* dynamic LDS per workgroup */
    int optimised;       /* 1: optimised round schedule (sparse partial rounds, normalised layers), 0: the reference's dense one */
    int row_tables;      /* 1: t-term matrix rows consume shifted tables (81 t + 18 multiplies), 0: element form (81 t + 81);
                          * window engines: how the history terms of the S-box inputs are formed - 1 shifted tables, 2 rows on the matrix cores */
    int lane_tables;     /* always 0 (no engine updates sparse layers through shifted tables any more); kept for the ABI */
    int mfma_dense;      /* 1: rows of the dense layers come from the matrix cores (int8 GEMM, pmx_mfma.hpp) */
    int launches;        /* kernel launches of the call: 1, or the passes of an absorb / squeeze call on wide states (and on device-filling t = 3 calls) */
    int partial_window;  /* K > 0: the partial rounds run as windows of K S-boxes, each closed by ONE layer on the matrix cores
                            (no sparse layers on the VALU); 0: one sparse layer per partial round */
} pmx_engine_info;
int pmx_ctx_engine_info(const pmx_ctx *ctx, int op, size_t n, size_t len, pmx_engine_info *out);

/* ---- permutation ------------------------------------------------------------------------------
 * PoseidonSponge::permute (src/poseidon/mod.rs:95-118 with apply_ark :76-80, apply_s_box :63-74,
 * apply_mds :82-93) applied independently to n states, in place.  states: [n][t][4].
 * The host variant copies in, runs the kernel, copies out.  The _dev variant takes a device pointer
 * and a hipStream_t (NULL = default stream) and only enqueues: one launch, nothing allocated; it may be captured into a graph.  */
int pmx_permute_batch(pmx_ctx *ctx, uint64_t *states, size_t n);
int pmx_permute_batch_dev(pmx_ctx *ctx, uint64_t *d_states, size_t n, void *stream);

/* ---- fixed-shape hash driver ------------------------------------------------------------------
 * Per row: PoseidonSponge::new; absorb(in_len native elements); squeeze_native_field_elements(out_len)
 * (src/poseidon/mod.rs:219-254, 321-341).  in: [n][in_len][4], out: [n][out_len][4].  in_len may be 0
 * (absorb of an empty input is a no-op, mod.rs:234-236).  The _dev variant is one launch on the caller's stream, nothing allocated; it may
 * be captured into a graph. */
int pmx_hash_batch(pmx_ctx *ctx, const uint64_t *in, size_t in_len, uint64_t *out, size_t out_len, size_t n);
int pmx_hash_batch_dev(pmx_ctx *ctx, const uint64_t *d_in, size_t in_len, uint64_t *d_out, size_t out_len,
                       size_t n, void *stream);

/* ---- duplex sponge driver on explicit (state, mode) ---------------------------------------------
 * n mid-stream sponges as moved out by SpongeExt::into_state (src/lib.rs:188-195,
 * src/poseidon/mod.rs:344-367): states [n][t][4], mode_tag [n], mode_index [n]; all updated in place.
 * absorb: CryptographicSponge::absorb for in_len native elements per sponge (mod.rs:232-254, 121-150).
 * squeeze: FieldBasedCryptographicSponge::squeeze_native_field_elements(out_len) (mod.rs:321-341,
 * 153-182, including the `!= rate` test of :175).  Sponges in one call may be in different modes.
 * Widths 4..9 (and width 3 from 32769 sponges up) run a call as PASSES on the permutation engine of the width (one launch per
 * permutation a sponge of the batch can need, ceil(len / rate); a sponge is permuted exactly as often as the reference would
 * permute it).  A _dev call moves at most 65536 rates of elements per sponge, whatever the width and the batch size (PMX_ERR_ARG
 * beyond: split the call - to a duplex sponge two calls are the same as one, except that a squeeze must not be cut so that a piece of
 * exactly `rate` elements meets a sponge inside its rate, mod.rs:175).  The HOST-buffer entry points take any length, as the reference
 * does: they cut a longer call into such pieces themselves.
 * The _dev variants only enqueue on the caller's stream, with two provisos for the pass form: (1) the pass lists live in device
 * blocks the context keeps in a pool (a call takes the block its stream used last, or one whose earlier use has completed - the
 * context's own event says so -, or allocates one: calls on different streams stay independent; concurrent calls of ONE context
 * serialise while they enqueue).  An allocation (hipMalloc) may therefore happen inside the call: these two entry points must not
 * be captured into a hipGraph.  (2) A stream must outlive the driver work pending on it: synchronise it before destroying it. */
int pmx_sponge_absorb_batch(pmx_ctx *ctx, uint64_t *states, uint32_t *mode_tag, uint32_t *mode_index,
                            const uint64_t *in, size_t in_len, size_t n);
int pmx_sponge_squeeze_batch(pmx_ctx *ctx, uint64_t *states, uint32_t *mode_tag, uint32_t *mode_index,
                             uint64_t *out, size_t out_len, size_t n);
/* Device-resident mode words need their natural alignment (4 bytes) and are not validated: absorb takes an index above the rate as the rate and any tag other than
 * PMX_MODE_ABSORBING as PMX_MODE_SQUEEZING, and (in_len > 0) writes back PMX_MODE_ABSORBING. */
int pmx_sponge_absorb_batch_dev(pmx_ctx *ctx, uint64_t *d_states, uint32_t *d_mode_tag, uint32_t *d_mode_index,
                                const uint64_t *d_in, size_t in_len, size_t n, void *stream);
/* Likewise squeeze takes an index above the rate as the rate and any tag other than PMX_MODE_SQUEEZING as PMX_MODE_ABSORBING,
 * and writes back PMX_MODE_SQUEEZING. */
int pmx_sponge_squeeze_batch_dev(pmx_ctx *ctx, uint64_t *d_states, uint32_t *d_mode_tag, uint32_t *d_mode_index,
                                 uint64_t *d_out, size_t out_len, size_t n, void *stream);

/* ---- variable-length rows ----------------------------------------------------------------------
 * The hash and absorb drivers with a length per row (the reference's absorb takes any number of elements per sponge and call,
 * src/poseidon/mod.rs:232-254 with absorb_internal :121-150).  Row i of `in` is the elements in[offsets[i] .. offsets[i+1])
 * ([*][4] u64, Montgomery form, as everywhere); offsets: [n+1] u64, non-decreasing.  Rows may be empty.
 * hash, row i: PoseidonSponge::new; absorb(row i); squeeze_native_field_elements(out_len) (mod.rs:219-230, 232-254, 321-341);
 *   out: [n][out_len][4].  An empty row gives what pmx_hash_batch gives with in_len = 0.  The squeeze is the driver's above: out_len
 *   is at most 65536 rates (PMX_ERR_ARG beyond).
 * absorb, sponge i: CryptographicSponge::absorb(row i) on (states[i], mode_tag[i], mode_index[i]), any mode.  A sponge whose row is
 *   empty is left completely untouched - state, tag and index - also when it is Squeezing or at Absorbing{rate}: the reference
 *   returns before the mode match (mod.rs:234-236).
 * Host entries: offsets and mode words are validated (PMX_ERR_ARG naming the first bad row, before anything is modified); only
 *   in[offsets[0] .. offsets[n]) is uploaded; rows of any length (a row longer than 65536 rates is absorbed in pieces - the same thing
 *   to a duplex sponge - with the states kept on the device in between).
 * _dev entries: max_len is the caller's bound on every row's length.  It sets the number of passes and is subject to the 65536-rate
 *   limit of the fixed _dev driver (PMX_ERR_ARG beyond, nothing launched).  Device-resident offsets are not validated (like
 *   device-resident mode words): a decreasing pair reads as an empty row, and a row longer than max_len is absorbed up to max_len
 *   elements.  d_offsets needs the natural alignment of uint64_t (8 bytes).  Alignment, the n limits and the provisos of the fixed _dev driver above hold (the pass lists and - for the hash - the n
 *   fresh states and mode words come from the context's per-stream pool: not to be captured into a hipGraph). */
int pmx_hash_varlen_batch(pmx_ctx *ctx, const uint64_t *in, const uint64_t *offsets, uint64_t *out, size_t out_len, size_t n);
int pmx_hash_varlen_batch_dev(pmx_ctx *ctx, const uint64_t *d_in, const uint64_t *d_offsets, size_t max_len, uint64_t *d_out,
                              size_t out_len, size_t n, void *stream);
int pmx_sponge_absorb_varlen_batch(pmx_ctx *ctx, uint64_t *states, uint32_t *mode_tag, uint32_t *mode_index, const uint64_t *in,
                                   const uint64_t *offsets, size_t n);
int pmx_sponge_absorb_varlen_batch_dev(pmx_ctx *ctx, uint64_t *d_states, uint32_t *d_mode_tag, uint32_t *d_mode_index,
                                       const uint64_t *d_in, const uint64_t *d_offsets, size_t max_len, size_t n, void *stream);

/* ---- squeeze bytes and bits ----------------------------------------------------------------------
 * CryptographicSponge::squeeze_bytes / squeeze_bits (src/poseidon/mod.rs:256-286) on n sponges held as (state, mode) like the drivers
 * above.  With B the bit length of the context's modulus (MODULUS_BIT_SIZE; this library takes 2^224 < p < 2^255):
 * bytes: u = (B - 1) / 8 (28 .. 31), E = ceil(num_bytes / u): squeeze E native elements; each contributes the first u bytes of its
 *   canonical integer in little-endian order (into_bigint().to_bytes_le()[..u], mod.rs:257-268); the concatenation is truncated to
 *   num_bytes.  out: [n][num_bytes], rows packed without padding.
 * bits: u = B - 1 (224 .. 254), E = ceil(num_bits / u), bits little-endian (to_bits_le()[..u], mod.rs:274-285), truncated to num_bits.
 *   out: [n][num_bits], ONE BYTE PER BIT holding 0 or 1 - the memory of a Rust Vec<bool>, passed as it stands.
 * States and mode words end exactly as after pmx_sponge_squeeze_batch[_dev] with out_len = E on the same sponges, E = 0 included (that
 * call still permutes an Absorbing sponge, mod.rs:324-328; so does this one).  Sponges of one call may be in different modes.
 * The canonical integer comes from the ABI residue by one Montgomery reduction on the device (no host pass over the elements, and only
 * n * num_bytes bytes cross the link from the host entries).  Squeezed elements are reduced, so the question does not arise here, but
 * the conversion itself takes any 256-bit word modulo p.
 * _dev: d_out needs NO alignment (num_bytes may be odd: rows start at any address); states and mode words as for the native _dev squeeze.
 *   A call writes [d_out, d_out + n * num_bytes) and nothing else of the caller's.  E is subject to the 65536-rate limit of the native
 *   _dev squeeze (PMX_ERR_ARG beyond, nothing launched).  Only enqueues; the E native elements pass through a scratch block of the
 *   context's per-stream pool (the provisos of the _dev drivers above hold: not to be captured into a hipGraph).  The block is at most
 *   PMX_SQUEEZE_SCRATCH_BYTES, or E * 32 bytes if one sponge needs more: a call with n * E * 32 above it runs in slices over sponges.
 * Host entries: mode words are validated; any length (a call beyond 65536 rates of elements is cut on element boundaries with the rule
 *   of the native host squeeze: never a last piece of exactly one rate).
 * To the engine choice this is a PMX_OP_SQUEEZE of E elements: pmx_ctx_engine_info(ctx, PMX_OP_SQUEEZE, n, E) names the engine; its
 * `launches` does not count the conversion launch (one per slice). */
#define PMX_SQUEEZE_SCRATCH_BYTES ((size_t)64 << 20)
int pmx_sponge_squeeze_bytes_batch(pmx_ctx *ctx, uint64_t *states, uint32_t *mode_tag, uint32_t *mode_index, uint8_t *out,
                                   size_t num_bytes, size_t n);
int pmx_sponge_squeeze_bytes_batch_dev(pmx_ctx *ctx, uint64_t *d_states, uint32_t *d_mode_tag, uint32_t *d_mode_index, uint8_t *d_out,
                                       size_t num_bytes, size_t n, void *stream);
int pmx_sponge_squeeze_bits_batch(pmx_ctx *ctx, uint64_t *states, uint32_t *mode_tag, uint32_t *mode_index, uint8_t *out,
                                  size_t num_bits, size_t n);
int pmx_sponge_squeeze_bits_batch_dev(pmx_ctx *ctx, uint64_t *d_states, uint32_t *d_mode_tag, uint32_t *d_mode_index, uint8_t *d_out,
                                      size_t num_bits, size_t n, void *stream);

/* ---- proof-of-work grinding ------------------------------------------------------------------------
 * The grinding step of a FRI / STARK transcript: find a nonce whose absorption makes the transcript squeeze `bits` zero bits.  About 2^bits
 * independent permutations of ONE sponge state; the candidates exist only in registers.  (No counterpart in the reference; the acceptance
 * rule is defined through its absorb and squeeze_bits, src/poseidon/mod.rs:232-254, 272-286.)
 * Inputs: a sponge (state [t][4], mode_tag, mode_index) of the context's config, a difficulty `bits`, a nonce range [first, first + count).
 * A nonce v (a uint64_t) is ACCEPTED iff
 *     c = sponge.clone(); c.absorb(&F::from(v)); c.squeeze_bits(bits) is all false.
 * With B the bit length of the modulus and bits <= B - 1 that is: the low `bits` bits of the canonical integer of the first squeezed
 * element are zero.  In permutations:
 *   Absorbing{i}, i < rate:           add the ABI residue of v (v * 2^256 mod p, what F::from(v) holds) into state[capacity + i], permute
 *                                     once, test state[capacity].
 *   Absorbing{rate} or Squeezing{any}: the reference permutes before it absorbs (mod.rs:239-252).  That permutation does not depend on v:
 *                                     it is done ONCE for the whole search, and the rule is then the case above with i = 0.
 * Result: *found_out = 1 and *nonce_out = the SMALLEST accepted nonce of the range, or *found_out = 0 (*nonce_out is then not written).
 *   Deterministic whatever the launch geometry.  The caller's sponge is not modified: the caller absorbs the winning nonce with the
 *   entries above (pmx_sponge_absorb_batch with n = 1 and the element F::from(nonce)).
 * Host-buffer entry only: one state goes up and one word comes down, so device residency buys nothing.  It serialises on the context's
 *   host lock like every host-buffer entry and runs inside the catch-all.  The range is searched in chunks of 2^21 candidates (measured:
 *   profiles/grind/README.md), in ascending order, one launch each; the search stops behind the first chunk that reports a hit.
 * Errors (PMX_ERR_ARG, nothing launched): a null pointer; a mode word the host drivers refuse (a tag that is neither mode, an index above the
 *   rate); bits > B - 1 (a second squeezed element would be needed); first + count > 2^64.
 * count = 0: PMX_OK, *found_out = 0, nothing launched.  bits = 0: every nonce is accepted - *nonce_out = first, nothing launched.
 * Engine: pmx_ctx_engine_info(ctx, PMX_OP_GRIND, n, 0) names the engine of a chunk of n candidates; the choice is that of a 2-to-1
 *   compression of n parents (the quad engine for the split (rate 2, capacity 1) of t = 3 up to 32768 candidates, the window engines for
 *   t = 3 .. 9, the run-time-width engine otherwise).
 * What this family lacks: there is no *_dev entry - a capturable form on device-resident state and result words comes later, together with
 *   its stream and capture tests -, no batch of sponges in one call and no device-group form. */
int pmx_sponge_grind(pmx_ctx *ctx, const uint64_t *state /*[t][4], host*/, uint32_t mode_tag, uint32_t mode_index,
                     uint32_t bits, uint64_t first, uint64_t count, uint64_t *nonce_out, int *found_out);

/* ---- 2-to-1 Merkle compression ------------------------------------------------------------------
 * parent = (new; absorb([left, right]); squeeze_native(1))[0]  (needs rate >= 2), level by level.
 * leaves: [n_leaves][4], n_leaves a power of two.  nodes (may be NULL): [2*n_leaves-1][4] receives the
 * leaves, then every level, root last.  root (may be NULL): [4]. */
int pmx_merkle_2to1(pmx_ctx *ctx, const uint64_t *leaves, size_t n_leaves, uint64_t *nodes, uint64_t *root);
/* Device variant: d_nodes [2*n_leaves-1][4] must already hold the leaves in its first n_leaves rows.  One launch per level on the caller's
 * stream, nothing allocated; it may be captured into a graph. */
int pmx_merkle_2to1_dev(pmx_ctx *ctx, uint64_t *d_nodes, size_t n_leaves, void *stream);

/* n_trees independent 2-to-1 trees of leaves_per_tree leaves each (a power of two; n_trees is any number >= 1), advanced
 * TOGETHER level by level: the narrow top levels of one tree are latency-bound (a level of <= 16384 compressions costs one
 * permutation's dependent chain whatever its width), a level of the forest is n_trees times as wide.  Layout, level-major:
 * leaves: [n_trees][leaves_per_tree][4] (tree after tree); nodes (may be NULL): [n_trees * (2*leaves_per_tree - 1)][4] receives
 * the leaves, then level 1 of every tree (tree after tree), ..., then the n_trees roots; roots (may be NULL): [n_trees][4].
 * Tree b's node j of level l (level 0 = leaves, m = leaves_per_tree) is row  n_trees*(2m - 2m/2^l) + b*(m/2^l) + j.
 * The device variant takes d_nodes with the leaves in its first n_trees*leaves_per_tree rows and only enqueues (one launch per level,
 * nothing allocated; it may be captured into a graph).
 * (No counterpart in the reference: a parent is new; absorb([l, r]); squeeze_native(1) as above.) */
int pmx_merkle_2to1_forest(pmx_ctx *ctx, const uint64_t *leaves, size_t n_trees, size_t leaves_per_tree, uint64_t *nodes,
                           uint64_t *roots);
int pmx_merkle_2to1_forest_dev(pmx_ctx *ctx, uint64_t *d_nodes, size_t n_trees, size_t leaves_per_tree, void *stream);

/* Authentication paths over the node array pmx_merkle_2to1 produces ([2*n_leaves-1][4]: leaves, then every level, root
 * last).  The container itself lives upstream (ark-crypto-primitives), not in arkworks-rs/sponge; a parent is
 * (new; absorb([left, right]); squeeze_native(1))[0] as above.  depth = log2(n_leaves).
 * pmx_merkle_paths: host-only gather - paths_out [k][depth][4] receives, for each indices[i], the sibling of the leaf and
 * of each ancestor, bottom-up.  Every index is checked before anything is written (as pmx_merkle_ary_paths and
 * pmx_merkle_ragged_paths do): a call refused with "out of range" leaves paths_out untouched.
 * pmx_merkle_verify_paths: k paths at once - one upload, `depth` level steps on the device (each a batched 2-to-1
 * compression of all k running nodes), one download: ok_out[i] = 1 iff hashing leaves[i] up its path (indices[i] says
 * left / right at each level) gives `root` and indices[i] < 2^depth.
 * pmx_merkle_verify_paths_dev: the same on device-resident buffers, enqueue only (a device-to-device copy, two launches per level, one for
 * the verdicts; nothing allocated: it may be captured into a graph); d_work is [k][12] u64 of scratch.  d_leaves, d_paths,
 * d_root and d_work are 16-byte aligned like every array of elements; d_indices needs 8 bytes, d_ok (k single bytes) any address. */
int pmx_merkle_paths(const uint64_t *nodes, size_t n_leaves, const uint64_t *indices, size_t k, uint64_t *paths_out);
int pmx_merkle_verify_paths(pmx_ctx *ctx, const uint64_t *leaves, const uint64_t *indices, const uint64_t *paths, size_t depth,
                            size_t k, const uint64_t root[PMX_LIMBS], uint8_t *ok_out);
int pmx_merkle_verify_paths_dev(pmx_ctx *ctx, const uint64_t *d_leaves, const uint64_t *d_indices, const uint64_t *d_paths,
                                size_t depth, size_t k, const uint64_t *d_root, uint8_t *d_ok, uint64_t *d_work, void *stream);

/* ---- Merkle trees of any arity ---------------------------------------------------------------------
 * The width people choose so that ONE permutation compresses `rate` children (octal trees at t = 9, quaternary at t = 5):
 *   parent = (new; absorb([c_0 .. c_{arity-1}]); squeeze_native(1))[0]
 *          = permute(state[capacity + j] = c_j for j < arity, every other element 0)[capacity]          for 2 <= arity <= rate,
 * because absorbing at most `rate` elements into a fresh sponge permutes exactly once, at the squeeze (src/poseidon/mod.rs:126-135,
 * 219-230, 324-328).  A tree of N leaves costs (N - 1) / (arity - 1) permutations and log_arity(N) levels.  arity 2 is the 2-to-1
 * compression above: at arity 2 every array here is byte for byte what the pmx_merkle_2to1* / pmx_merkle_paths /
 * pmx_merkle_verify_paths* entries produce and accept, and the same kernels run.  (No counterpart in the reference.)
 * Shapes: n_leaves = arity^depth with depth >= 0 (one leaf is its own root, nothing is launched); pmx_merkle_ary_shape (host only)
 *   gives depth and n_nodes = (arity^(depth+1) - 1) / (arity - 1), and refuses what every entry below refuses: arity < 2, a leaf count
 *   that is no power of the arity, a node array whose byte size overflows size_t (PMX_ERR_ARG).
 * nodes: [n_nodes][4], the leaves, then every level, root last; the _dev variants take d_nodes with the leaves in its first rows
 *   and only enqueue.  nodes / root / roots may be NULL in the host entries.
 * Capture: every _dev entry of this family (pmx_merkle_ary_dev, _forest_dev, _paths_dev, _verify_paths_dev) launches on the caller's stream
 *   only and allocates nothing; each may be captured into a graph.
 * Forest, level-major like pmx_merkle_2to1_forest: level l of every tree, tree after tree.  With m = leaves_per_tree, tree b's node j
 *   of level l is row  n_trees * (m + m/arity + ... + m/arity^(l-1)) + b * (m / arity^l) + j;  the last n_trees rows are the roots.
 * Paths: [k][depth][arity - 1][4], bottom-up; per level the siblings in child order with the running node's own slot left out (the
 *   running node is child (index / arity^level) % arity of its parent).
 *   pmx_merkle_ary_paths: host-only gather over a node array; an index >= n_leaves is PMX_ERR_ARG and nothing is written.
 *   pmx_merkle_ary_paths_dev: the same gather on the device, enqueue only - node array, indices and paths stay there.  Device-resident
 *     indices are not validated: an index >= n_leaves gets an all-zero path (and fails verification by its range).
 * Verification: ok[i] = 1 iff hashing leaves[i] up its path gives `root` and indices[i] < arity^depth.  One compression launch of all
 *   k running nodes per level; d_work is [k][(arity + 1) * 4] u64 of scratch.
 * Errors, nothing launched or written on any: PMX_ERR_ARG for arity < 2, a leaf count that is no power of the arity, byte sizes that
 *   overflow, arity^depth beyond 64 bits, null pointers, an element array (d_nodes, d_leaves, d_paths, d_root, d_work) that is not
 *   16-byte aligned (d_indices needs 8 bytes, d_ok any address); PMX_ERR_CONFIG for arity > rate: more children than the rate is a
 *   hash row (pmx_hash_batch_dev with in_len = arity, out_len = 1), not a single compression.
 * Engine: pmx_ctx_engine_info(ctx, PMX_OP_COMPRESS, n, len) names the engine of a level of n parents; len is the arity and does not
 *   enter the choice (len 0 .. 2: the 2-to-1 launch, which alone can run on the quad engine - it needs rate 2). */
int pmx_merkle_ary_shape(size_t n_leaves, uint32_t arity, size_t *depth, size_t *n_nodes);
int pmx_merkle_ary(pmx_ctx *ctx, const uint64_t *leaves, size_t n_leaves, uint32_t arity, uint64_t *nodes, uint64_t *root);
int pmx_merkle_ary_dev(pmx_ctx *ctx, uint64_t *d_nodes, size_t n_leaves, uint32_t arity, void *stream);
int pmx_merkle_ary_forest(pmx_ctx *ctx, const uint64_t *leaves, size_t n_trees, size_t leaves_per_tree, uint32_t arity,
                          uint64_t *nodes, uint64_t *roots);
int pmx_merkle_ary_forest_dev(pmx_ctx *ctx, uint64_t *d_nodes, size_t n_trees, size_t leaves_per_tree, uint32_t arity, void *stream);
int pmx_merkle_ary_paths(const uint64_t *nodes, size_t n_leaves, uint32_t arity, const uint64_t *indices, size_t k,
                         uint64_t *paths_out);
int pmx_merkle_ary_paths_dev(pmx_ctx *ctx, const uint64_t *d_nodes, size_t n_leaves, uint32_t arity, const uint64_t *d_indices,
                             size_t k, uint64_t *d_paths, void *stream);
int pmx_merkle_ary_verify_paths(pmx_ctx *ctx, const uint64_t *leaves, const uint64_t *indices, const uint64_t *paths, size_t depth,
                                uint32_t arity, size_t k, const uint64_t root[PMX_LIMBS], uint8_t *ok_out);
int pmx_merkle_ary_verify_paths_dev(pmx_ctx *ctx, const uint64_t *d_leaves, const uint64_t *d_indices, const uint64_t *d_paths,
                                    size_t depth, uint32_t arity, size_t k, const uint64_t *d_root, uint8_t *d_ok, uint64_t *d_work,
                                    void *stream);

/* ---- leaf updates of a tree of any arity ------------------------------------------------------------
 * k leaves of a tree change and only their ancestors are recomputed: at most k * depth permutations instead of the (N - 1) / (arity - 1)
 * of a rebuild (the 8-ary tree over 2^21 leaves with k = 1024: at most 7 168 instead of 299 593).  The node array is the one
 * pmx_merkle_ary[_dev] produces ([n_nodes][4]: leaves, then every level, root last; at arity 2 also the array of pmx_merkle_2to1*).
 * Afterwards it is byte for byte what pmx_merkle_ary gives over the leaf row with new_leaves[i] at indices[i]; a node that is no
 * ancestor of an updated leaf is not written at all (but see the whole levels of the device entry).
 * pmx_merkle_ary_update_dev: everything device-resident, on the caller's stream.  It only enqueues and allocates nothing, so - unlike
 *   the sponge drivers - it may be captured into a graph.  d_work is [k][(arity + 1) * 4] u64 of scratch, as for
 *   pmx_merkle_ary_verify_paths_dev.  d_nodes, d_new_leaves and d_work are 16-byte aligned, d_indices 8-byte.  The new leaves are
 *   scattered into the leaf rows; then, level by level, while k is below the number W of parents the level has: the arity children of
 *   every update's parent are gathered, one compression launch of k rows runs, and the k digests are scattered to their parents (two
 *   updates under one parent compute it twice and store identical bytes).  From the first level with k >= W on, that level and every
 *   level above it run as the whole-level launches of pmx_merkle_ary_dev, which rewrite every node of those levels with the value it
 *   has: an update never costs more permutations than a rebuild.
 *   Device-resident indices are not validated.  An index >= n_leaves is ignored: its leaf and its ancestors are not written, and
 *   nothing outside the arrays is read or written.  Indices must be distinct, or equal with equal leaves: two different leaves for one
 *   index leave that leaf row unspecified (its two 16-byte halves may come from different updates); the tree above it is still the tree
 *   of whatever landed.
 *   n_leaves = 1: the leaf is the root, only the scatter runs.  k = 0: PMX_OK, nothing launched.
 * pmx_merkle_ary_update: `nodes` is a host array and is not uploaded.  Every index is validated before anything is modified (an index
 *   >= n_leaves is PMX_ERR_ARG naming it); duplicates are sequential updates, the last one wins.  The host packs the children rows of
 *   the distinct ancestors of every level, one upload takes them to the device, each level is one compression launch and one scatter
 *   of its digests into the next level's rows, one download brings all digests back; then leaves and digests are written into `nodes`
 *   and the root into `root` (may be NULL).  Each distinct ancestor is permuted once.  A failure leaves `nodes` untouched.
 * Errors, nothing launched or written on any: those of pmx_merkle_ary_paths_dev (PMX_ERR_ARG for arity < 2, a leaf count that is no power
 *   of the arity, byte sizes that overflow, null pointers, misaligned device pointers, "batch too large" by the bounds of
 *   pmx_merkle_ary_verify_paths_dev); PMX_ERR_CONFIG for arity > rate. */
int pmx_merkle_ary_update_dev(pmx_ctx *ctx, uint64_t *d_nodes, size_t n_leaves, uint32_t arity, const uint64_t *d_indices,
                              const uint64_t *d_new_leaves, size_t k, uint64_t *d_work, void *stream);
int pmx_merkle_ary_update(pmx_ctx *ctx, uint64_t *nodes, size_t n_leaves, uint32_t arity, const uint64_t *indices,
                          const uint64_t *new_leaves, size_t k, uint64_t *root /* may be NULL */);

/* ---- Merkle trees over any number of leaves -----------------------------------------------------------
 * pmx_merkle_ary* takes arity^depth leaves only; people commit to 2^k rows, or to however many they have.  For 2 <= arity <= rate and any
 * n_leaves >= 1: level 0 is the leaves (M_0 = n_leaves), level l + 1 has M_{l+1} = ceil(M_l / arity) nodes, and the first level of width
 * 1 is the root; depth = the levels above the leaves (n_leaves = 1: depth 0, the leaf is the root, nothing is launched).  Parent p of
 * level l + 1 absorbs the children p * arity .. min((p + 1) * arity, M_l) - 1 of level l:
 *   parent = (new; absorb(the r <= arity children that exist); squeeze_native(1))[0]
 *          = permute(state[capacity + j] = c_j for j < r, every other element 0)[capacity],
 * the reference sponge's own answer for a short row - absorb takes any number of elements, and at most `rate` of them into a fresh sponge
 * permute once, at the squeeze (src/poseidon/mod.rs:126-135, 219-230, 324-328).  A parent with ONE child is still a permutation, not a
 * promotion of the child.  (No counterpart in the reference.)
 * What the root does NOT bind: a short parent equals the parent of the same children padded with zero elements, so the root does not
 *   commit to n_leaves - the tree over n leaves and the tree over the same leaves followed by zero leaves up to the end of the last
 *   parent's row have one root.  A caller who needs the length bound binds it itself (in a leaf, or next to the root); verification
 *   takes n_leaves for this reason and accepts no index at or above it.
 * nodes: [n_nodes][4] as everywhere - the leaves, then every level, root last; n_nodes = sum of the M_l, level l starts at row
 *   M_0 + ... + M_{l-1}.  pmx_merkle_ragged_shape (host only) gives depth and n_nodes and refuses arity < 2, n_leaves = 0 and a node
 *   array whose byte size overflows size_t (PMX_ERR_ARG).  At n_leaves = arity^depth every array of this family is byte for byte what
 *   pmx_merkle_ary* produces and accepts and the same launches run; at arity 2 and a power of two the same holds for pmx_merkle_2to1*.
 * pmx_merkle_ragged: host buffers; nodes / root may be NULL.  pmx_merkle_ragged_dev: d_nodes holds the leaves in its first n_leaves rows;
 *   it only enqueues and allocates nothing (it may be captured like pmx_merkle_ary_dev): ONE compression launch per level, on the engine
 *   pmx_ctx_engine_info(ctx, PMX_OP_COMPRESS, W, arity) names for the level's W = M_{l+1} parents - at arity 2 too, the quad engine
 *   included; the short last row is bounded inside that launch and nothing at or beyond the level's end is read.
 * Paths: [k][depth][arity - 1][4] as for pmx_merkle_ary_paths; a sibling that does not exist (its index is at or beyond its level's
 *   width) is four zero words.  pmx_merkle_ragged_paths: host-only gather, an index >= n_leaves is PMX_ERR_ARG and nothing is written.
 *   pmx_merkle_ragged_paths_dev: the gather on the device, enqueue only (one launch, nothing allocated; it may be captured into a graph);
 *   an index >= n_leaves gets an all-zero path.
 * Verification: ok[i] = 1 iff hashing leaves[i] up its path gives `root` AND indices[i] < n_leaves.  The climb is that of
 *   pmx_merkle_ary_verify_paths* (absent siblings are zeros, so every row is a full one); d_work is [k][(arity + 1) * 4] u64.  depth must
 *   be the depth of (n_leaves, arity): PMX_ERR_ARG otherwise.  pmx_merkle_ragged_verify_paths_dev only enqueues and allocates nothing; it may
 *   be captured into a graph.
 * pmx_merkle_ragged_update_dev: the contract of pmx_merkle_ary_update_dev - enqueue only, nothing allocated (it may be captured), the same d_work, indices
 *   >= n_leaves ignored, whole-level launches from the first level with k >= W parents on; afterwards the array is byte for byte what a
 *   rebuild over the new leaves gives.  (There is no host-array pmx_merkle_ragged_update, no ragged forest and no device-group form.)
 * Errors, nothing launched or written on any: PMX_ERR_ARG for arity < 2, n_leaves = 0, byte sizes that overflow, a depth that is not the
 *   tree's, null pointers, an element array that is not 16-byte aligned (d_indices needs 8 bytes, d_ok any address), "batch too large" by
 *   the bounds of pmx_merkle_ary_verify_paths_dev; PMX_ERR_CONFIG for arity > rate. */
int pmx_merkle_ragged_shape(size_t n_leaves, uint32_t arity, size_t *depth, size_t *n_nodes);
int pmx_merkle_ragged(pmx_ctx *ctx, const uint64_t *leaves, size_t n_leaves, uint32_t arity, uint64_t *nodes, uint64_t *root);
int pmx_merkle_ragged_dev(pmx_ctx *ctx, uint64_t *d_nodes, size_t n_leaves, uint32_t arity, void *stream);
int pmx_merkle_ragged_paths(const uint64_t *nodes, size_t n_leaves, uint32_t arity, const uint64_t *indices, size_t k,
                            uint64_t *paths_out);
int pmx_merkle_ragged_paths_dev(pmx_ctx *ctx, const uint64_t *d_nodes, size_t n_leaves, uint32_t arity, const uint64_t *d_indices,
                                size_t k, uint64_t *d_paths, void *stream);
int pmx_merkle_ragged_verify_paths(pmx_ctx *ctx, const uint64_t *leaves, const uint64_t *indices, const uint64_t *paths, size_t depth,
                                   uint32_t arity, size_t n_leaves, size_t k, const uint64_t root[PMX_LIMBS], uint8_t *ok_out);
int pmx_merkle_ragged_verify_paths_dev(pmx_ctx *ctx, const uint64_t *d_leaves, const uint64_t *d_indices, const uint64_t *d_paths,
                                       size_t depth, uint32_t arity, size_t n_leaves, size_t k, const uint64_t *d_root, uint8_t *d_ok,
                                       uint64_t *d_work, void *stream);
int pmx_merkle_ragged_update_dev(pmx_ctx *ctx, uint64_t *d_nodes, size_t n_leaves, uint32_t arity, const uint64_t *d_indices,
                                 const uint64_t *d_new_leaves, size_t k, uint64_t *d_work, void *stream);

/* ---- Merkle trees of a fixed depth: empty positions are default leaves, leaves are appended in place ---
 * Note-commitment trees, identity groups and rollup state trees are INCREMENTAL trees: arity k (2 <= k <= rate), a fixed depth D
 * (1 <= D <= 64, k^D <= 2^64), leaves appended left to right, every position not yet filled counting as a default leaf e[0] and an empty
 * subtree of height l as e[l] = (new; absorb(k copies of e[l-1]); squeeze_native(1))[0].  The tree over n leaves, 0 <= n <= k^D, is BY
 * DEFINITION pmx_merkle_ary over the leaf row padded with e[0] to k^D leaves - which at depth 32 nobody can hold.  (No counterpart in the
 * reference, which has no tree.)
 * Node j of level l is complete iff (j + 1) k^l <= n and partial iff it is not complete and j k^l < n; a level has at most one partial
 *   node.  The frontier is, per level l < D, the complete nodes k floor(f_l / k) .. f_l - 1 with f_l = floor(n / k^l): digit l of n in base
 *   k of them.  frontier: [D][k - 1][4]; slots at or beyond the digit are zero words on output and ignored on input, so equal trees have
 *   equal frontier bytes.  (frontier, n) is all a caller keeps: D (k - 1) digests and a count.
 * pmx_merkle_fixed_defaults: defaults_out [D + 1][4] = e[0 .. D] from the caller's default leaf; D dependent launches of one unit, done once.
 * pmx_merkle_frontier_append: m new leaves behind the n_leaves the frontier stands for.  Per level ONE full-row compression launch, on
 *   the engine pmx_ctx_engine_info(ctx, PMX_OP_COMPRESS, parents, arity) names (arity 2: the 2-to-1 launch, the quad engine included),
 *   over a row that holds the level's frontier nodes, its newly complete nodes (level 0: the new leaves), its partial node and copies of
 *   e[l] up to a multiple of k; the pads and the frontier nodes of all levels are laid out by one launch before the walk, the new
 *   frontier and the root come back in one download: at most D compression launches per piece, nothing per leaf, no short row.  A long
 *   append runs in pieces of a bounded number of leaves; appends compose exactly, so pieces change no byte.  frontier_in may be NULL
 *   iff n_leaves = 0; frontier_out may alias frontier_in; root (may be NULL) receives node 0 of level D, which is a complete node only
 *   when n_leaves + m = k^D.  m = 0 is legal and returns the current root - except over a FULL tree, whose frontier holds no node: with
 *   n_leaves = k^D and m = 0 a non-NULL root is PMX_ERR_ARG.
 * pmx_merkle_fixed_shape (host only): the dense form stores max(1, ceil(n_leaves / k^l)) nodes of level l = 0 .. D - the complete nodes
 *   and the partial one -, packed, leaves first and root last; n_leaves >= 1.
 * pmx_merkle_fixed: the dense form: the same walk from the empty frontier, every computed node kept (nodes [n_nodes][4] and root may be
 *   NULL).  At n_leaves = k^D the array is byte for byte that of pmx_merkle_ary.  `nodes` is written piece by piece.
 * pmx_merkle_fixed_paths (host only): paths_out [k_paths][D][k - 1][4] in the layout of pmx_merkle_ary_paths; a sibling beyond its
 *   level's stored width is e[l].  Every index is checked (< n_leaves) before anything is written.  The paths are accepted unchanged by
 *   pmx_merkle_ary_verify_paths(..., depth, arity, ...): there is no verifier of its own.
 * Like every host-buffer entry these serialise on the context's lock and run inside the catch-all; device scratch is the context's staging.
 * What the family lacks: host buffers only (no *_dev entry and no graph-capturable form), no forest and no device-group form.  Leaves of a
 *   fixed-depth tree are changed by pmx_merkle_update_witnesses below, from their openings; pmx_merkle_ary_update needs the dense array.
 * Errors, nothing launched or written on any: PMX_ERR_ARG for null pointers, arity < 2, depth = 0, depth > 64, k^D beyond 64 bits (k^D =
 *   2^64 is accepted), n_leaves + m > k^D, n_leaves = 0 of a dense tree, byte sizes that overflow size_t; PMX_ERR_CONFIG for arity > rate. */
int pmx_merkle_fixed_defaults(pmx_ctx *ctx, const uint64_t default_leaf[PMX_LIMBS], uint32_t arity, size_t depth,
                              uint64_t *defaults_out /* [depth + 1][4] */);
int pmx_merkle_frontier_append(pmx_ctx *ctx, uint32_t arity, size_t depth, const uint64_t *defaults,
                               const uint64_t *frontier_in /* may be NULL iff n_leaves == 0 */, size_t n_leaves, const uint64_t *new_leaves,
                               size_t m, uint64_t *frontier_out, uint64_t *root /* may be NULL */);
int pmx_merkle_fixed_shape(size_t n_leaves, uint32_t arity, size_t depth, size_t *n_nodes);
int pmx_merkle_fixed(pmx_ctx *ctx, const uint64_t *leaves, size_t n_leaves, uint32_t arity, size_t depth, const uint64_t *defaults,
                     uint64_t *nodes /* may be NULL */, uint64_t *root /* may be NULL */);
int pmx_merkle_fixed_paths(const uint64_t *nodes, size_t n_leaves, uint32_t arity, size_t depth, const uint64_t *defaults,
                           const uint64_t *indices, size_t k_paths, uint64_t *paths_out /* [k_paths][depth][arity - 1][4] */);

/* ---- sequential leaf updates of a fixed-depth tree, with witnesses --------------------------------------
 * A rollup or state-tree prover holds k updates (indices[j], new_leaves[j]) of a deep, sparsely filled tree and the opening of every
 * indices[j] in the tree as it stood BEFORE the batch; it needs the root after every update, the witness of every update - the opening of
 * indices[j] in the tree after updates 0 .. j - 1, which is what a circuit consumes - and the final root.  (No counterpart in the
 * reference, which has no tree.)
 * The tree: arity a (2 <= a <= rate), depth D (1 <= D <= 64, a^D <= 2^64), parent = (new; absorb(the a children); squeeze_native(1))[0],
 *   every row full, exactly as in pmx_merkle_ary: there is no short row.  Openings are [k][D][a - 1][4], bottom-up, per level the siblings
 *   in child order with the running node's own slot left out: the layout of pmx_merkle_ary_paths (and of pmx_merkle_fixed_paths).
 * Inputs: indices [k] (duplicates are allowed and are sequential updates of one leaf), new_leaves [k][4], paths [k][D][a - 1][4] - the
 *   opening of indices[j] in the OLD tree, the one before update 0, the same tree for every j.
 * The outputs are DEFINED by this model.  An overlay maps (level, node) to a value and starts empty.  For j = 0 .. k - 1, with
 *   q_l = indices[j] / a^l:  v_0 = new_leaves[j];  for l = 0 .. D - 1 the sibling c of q_l in slot s is overlay[(l, c)] if present, else
 *   paths[j][l][s] - that value is witness[j][l][s] -, and v_{l+1} is the parent of the row with v_l at digit q_l mod a and the siblings
 *   around it;  then overlay[(l, q_l)] = v_l for all l <= D, and roots[j] = v_D.
 *   When `paths` are the true openings of one tree, witness[j] is the true opening of indices[j] in the tree after j updates and roots[j]
 *   the true root after update j.  The call does NOT check `paths` against an old root: that check is pmx_merkle_ary_verify_paths,
 *   unchanged (old leaves, indices, paths, D, a, old root).  Inconsistent paths still give exactly the model's bytes.
 * The work is not sequential by level: once a level is known, the next is k independent compressions.  The host computes, per level, for
 *   every sibling the last earlier update that wrote it (one sort, then O(k a) per level); per level one gather launch builds the k rows
 *   and the level's witnesses, and ONE full-row compression launch of k rows follows, on the engine pmx_ctx_engine_info(ctx,
 *   PMX_OP_COMPRESS, k, a) names (arity 2: the 2-to-1 launch, the quad engine included): D compression launches, k D permutations.  Device
 *   memory is O(k a) elements whatever D: a level's slab of the openings goes up, and its slab of the witnesses comes down, as one 2-D
 *   copy, the next level's while this one compresses.
 * witness_out [k][D][a - 1][4], roots_out [k][4] and root [4] (= roots[k - 1]) may each be NULL; the others receive the same bytes.
 * k = 0: PMX_OK, nothing launched; a non-NULL root is then PMX_ERR_ARG, because no root exists to return.  k is at most 2^32 - 2.
 * Host buffers only (no *_dev entry); like every host-buffer entry it serialises on the context's lock and runs inside the catch-all.
 * Errors, nothing launched or written on any: PMX_ERR_ARG for null pointers, arity < 2, depth = 0, depth > 64, a^D beyond 64 bits (a^D =
 *   2^64 is accepted), an index >= a^D (the message names it), byte sizes that overflow size_t, k > 2^32 - 2 ("batch too large");
 *   PMX_ERR_CONFIG for arity > rate. */
int pmx_merkle_update_witnesses(pmx_ctx *ctx, uint32_t arity, size_t depth, const uint64_t *indices, const uint64_t *new_leaves,
                                const uint64_t *paths, size_t k, uint64_t *witness_out /* may be NULL: [k][depth][arity - 1][4] */,
                                uint64_t *roots_out /* may be NULL: [k][4] */, uint64_t *root /* may be NULL: [4], = roots[k - 1] */);

/* ---- matrix commitments: the rows of a trace / LDE matrix as the leaves of a tree ---------------------
 * A prover holds a matrix of n_rows rows and row_len columns, almost always column-major (one column per polynomial), and commits to
 * its ROWS: leaf_i = (new; absorb(row i); squeeze_native(1))[0], the reference sponge's own answer for a row of any length - absorb
 * permutes whenever the rate is full and more input remains, the squeeze permutes once more (src/poseidon/mod.rs:121-150, 219-254,
 * 321-341) -, then the tree of pmx_merkle_ragged over the n_rows digests.  (No counterpart in the reference, which has no tree.)
 * matrix: [n_rows * row_len][4] host memory in one of the two layouts below; it is read where it lies, never transposed on the host.
 * Bytes: leaves_out is byte for byte pmx_hash_batch(the row-major copy of the matrix, in_len = row_len, out_len = 1); nodes / root are
 *   byte for byte pmx_merkle_ragged over those leaves ([n_nodes][4] and depth as pmx_merkle_ragged_shape(n_rows, arity) says; what the
 *   root does not bind is said there, and a row digest binds row_len no more than a sponge binds the length of what it absorbed:
 *   a row and the same row followed by zeros up to the next multiple of the rate have one digest); openings are
 *   pmx_merkle_ragged_paths on `nodes`, unchanged.  row_len may be any length >= 1 - rows longer than the rate are the point.
 * pmx_matrix_leaves: the digests alone.  pmx_matrix_commit: the digests land in the first n_rows rows of the device node array, the tree
 *   walk of pmx_merkle_ragged_dev follows on the same stream without the leaves leaving the device, one download brings back nodes
 *   and / or root (each may be NULL).
 * The link: the matrix goes up in slabs of rows of at most PMX_MATRIX_SLAB_BYTES each (65536 rows at least), through two slab buffers of the context - slab
 *   s + 1 is uploaded while slab s is hashed.  A column-major slab of rows [a, b) is one 2-D copy (b - a) * 32 bytes wide, row_len high,
 *   source pitch n_rows * 32, into a packed column-major buffer of leading dimension b - a; a row-major slab is one contiguous copy.
 *   One strided hash launch per slab (the units of a wave read consecutive elements of a column-major slab), on the engine
 *   pmx_ctx_engine_info(ctx, PMX_OP_HASH, b - a, row_len) names.  A page-locked matrix (pmx_host_alloc, hipHostRegister) is copied
 *   asynchronously from where it lies; a pageable one of at most 64 KiB goes through the context's page-locked staging block, one of
 *   16 MiB or more is page-locked for the length of the call, and what lies between takes the runtime's pageable staging.
 * pmx_matrix_rows: the k opened rows, a host-only gather: rows_out [k][row_len][4], each row contiguous (row-major) whatever the
 *   layout.  Every index is checked before anything is written (an index >= n_rows is PMX_ERR_ARG naming it).
 * pmx_matrix_verify_rows: ok[i] = 1 iff the digest of rows[i] ([k][row_len][4], as pmx_matrix_rows gives them) climbs paths[i] to
 *   `root` AND indices[i] < n_rows: one strided hash launch over the k rows, then the climb of pmx_merkle_ragged_verify_paths (paths
 *   [k][depth][arity - 1][4]; depth must be the depth of (n_rows, arity)).  k = 0: PMX_OK, nothing launched.
 * Like every host-buffer entry these serialise on the context's lock and run inside the catch-all.
 * What the family lacks: there is no device-resident form (no *_dev entry: a matrix that already lives on the device is hashed with
 *   pmx_hash_batch_dev, row-major only), no forest of matrices and no device-group form.
 * Errors, nothing launched or written on any: PMX_ERR_ARG for null pointers, n_rows = 0, row_len = 0, a layout that is neither of the
 *   two, byte sizes that overflow size_t, arity < 2, a depth that is not the tree's; PMX_ERR_CONFIG for arity > rate. */
#define PMX_MATRIX_ROW_MAJOR 0u   /* element (i, j) at matrix[(i * row_len + j) * 4] */
#define PMX_MATRIX_COL_MAJOR 1u   /* element (i, j) at matrix[(j * n_rows  + i) * 4] */
/* device memory of one upload slab (there are two), chosen from the sweep of profiles/matrix_commit/README.md: the smallest power of two
 * within 1 % of the best whole-call time for rows of 8 elements.  A slab never has fewer than 65536 rows (fewer leave the chip partly
 * empty whatever their bytes): rows longer than 16 elements take slabs of 65536 rows, 2 MiB per element of the row. */
#define PMX_MATRIX_SLAB_BYTES ((size_t)32 << 20)
int pmx_matrix_leaves(pmx_ctx *ctx, const uint64_t *matrix, size_t n_rows, size_t row_len, uint32_t layout, uint64_t *leaves_out);
int pmx_matrix_commit(pmx_ctx *ctx, const uint64_t *matrix, size_t n_rows, size_t row_len, uint32_t layout, uint32_t arity,
                      uint64_t *nodes /* may be NULL */, uint64_t *root /* may be NULL */);
int pmx_matrix_rows(const uint64_t *matrix, size_t n_rows, size_t row_len, uint32_t layout, const uint64_t *indices, size_t k,
                    uint64_t *rows_out);
int pmx_matrix_verify_rows(pmx_ctx *ctx, const uint64_t *rows, size_t row_len, const uint64_t *indices, const uint64_t *paths, size_t depth,
                           uint32_t arity, size_t n_rows, size_t k, const uint64_t root[PMX_LIMBS], uint8_t *ok_out);

/* ---- device groups: the batch sharded over the GPUs of one node -------------------------------------
 * The reference is single-threaded and has no distributed code; nothing in src/poseidon/mod.rs:62-183 couples one
 * sponge state to another, so n states are cut into `world` contiguous shards (pmx_shard_bounds), one per GPU, and
 * the permutation itself needs NO collective.  RCCL over xGMI is used for the final gather of the result shards
 * (to every rank: ncclAllGather, a group of ncclBroadcasts when n is not a multiple of world; to one rank, or piece by piece
 * behind the last step: grouped ncclSend / ncclRecv) and for the 32-byte subtree roots of the sharded Merkle reduction.
 *
 * A group is either all GPUs of ONE process (pmx_mgpu_create = ncclCommInitAll; this is what a Rust caller uses:
 * BatchPoseidon::new_multi in INTEGRATION.md) or ONE rank of a multi-process job (pmx_mgpu_create_rank =
 * ncclCommInitRank; rank 0 makes the id with pmx_mgpu_unique_id and the launcher carries it to the other ranks).
 * A group holds `n_local` devices with consecutive ranks first_rank .. first_rank + n_local - 1 of `world`.
 * Arrays indexed [local] below have n_local entries.  The *_dev calls enqueue on the group's own per-device
 * streams (pmx_mgpu_stream) and return; pmx_mgpu_synchronize waits for all of them.
 *
 * RCCL is bound when the first group is formed (dlopen of librccl.so.1 by SONAME - a process that already holds a copy
 * keeps it -, then /opt/rocm/lib/librccl.so.1).  The library reads no environment variable for this: a site's own RCCL
 * build is chosen the way any shared library is, through the loader's search path. */
#define PMX_UNIQUE_ID_BYTES 128
#define PMX_MAX_LOCAL_DEVICES 16
typedef struct pmx_mgpu pmx_mgpu;
typedef struct pmx_mgpu_info {
    int world;            /* ranks the group was created for */
    int n_local;          /* devices driven by this process */
    int first_rank;       /* rank of local device 0 */
    int width;            /* t = rate + capacity */
    int rccl_version;     /* ncclGetVersion, e.g. 22707 */
    int comm_ranks;       /* ncclCommCount of the LIVE communicator: proof that RCCL joined `world` ranks */
    int comm_first_rank;  /* ncclCommUserRank of local device 0 */
    int devices[PMX_MAX_LOCAL_DEVICES]; /* HIP device of each local slot */
} pmx_mgpu_info;

/* rank `rank` of `world` owns units [start, start + count) of n: contiguous, the first n % world shards one longer.
 * Pure host arithmetic (no device needed). */
int pmx_shard_bounds(size_t n, int world, int rank, size_t *start, size_t *count);
int pmx_mgpu_unique_id(uint8_t id[PMX_UNIQUE_ID_BYTES]);
/* devices: n_devices HIP device ordinals, or NULL for 0 .. n_devices-1 */
int pmx_mgpu_create(const pmx_config *cfg, int n_devices, const int *devices, pmx_mgpu **out);
int pmx_mgpu_create_rank(const pmx_config *cfg, int device, int rank, int world, const uint8_t id[PMX_UNIQUE_ID_BYTES],
                         pmx_mgpu **out);
int pmx_mgpu_destroy(pmx_mgpu *g);
int pmx_mgpu_get_info(const pmx_mgpu *g, pmx_mgpu_info *info);
void *pmx_mgpu_stream(const pmx_mgpu *g, int local);     /* hipStream_t of local device `local` (NULL if out of range) */
/* Its context (owned by the group).  Any other per-shard work - the hash driver, absorb, squeeze - is the single-device
 * *_dev entry point called with this context on pmx_mgpu_stream(g, local); pmx_mgpu_all_gather_dev then gathers the
 * per-row outputs with row_elems = out_len. */
pmx_ctx *pmx_mgpu_ctx(const pmx_mgpu *g, int local);
int pmx_mgpu_synchronize(pmx_mgpu *g);

/* PoseidonSponge::permute (src/poseidon/mod.rs:95-118) on n states in host memory, in place, sharded over the
 * group's devices (single-process groups): every device pipelines its own shard over PCIe, all devices at once. */
int pmx_mgpu_permute_batch(pmx_mgpu *g, uint64_t *states, size_t n);
/* pmx_hash_batch (per row: new; absorb(in_len); squeeze_native(out_len)) sharded the same way: rows [start, start+count)
 * of `in` and `out` go through device g's host path. */
int pmx_mgpu_hash_batch(pmx_mgpu *g, const uint64_t *in, size_t in_len, uint64_t *out, size_t out_len, size_t n);
/* The same on device-resident shards: d_shards[local] = [count][t][4] on that device, count from
 * pmx_shard_bounds(n_total, world, first_rank + local).  Only enqueues. */
int pmx_mgpu_permute_shards_dev(pmx_mgpu *g, uint64_t *const *d_shards, size_t n_total);
/* The final gather: d_all[local] = [n_total][row_elems][4] on every device receives all shards in rank order
 * (row_elems = t for states, 1 for digests).  RCCL; only enqueues.  (None of the pmx_mgpu_*_dev entries takes a stream: they run on the
 * group's own streams and are not meant for graph capture.) */
int pmx_mgpu_all_gather_dev(pmx_mgpu *g, const uint64_t *const *d_shards, uint64_t *const *d_all, size_t n_total,
                            size_t row_elems);
/* The gather to ONE rank: only `root` ends with all shards (d_all of its slot; the other slots' entries are not read and may be
 * NULL).  Every other rank sends its shard over its own link to the root - 1 / world of the all-gather's bytes per link.  Grouped
 * ncclSend / ncclRecv; only enqueues. */
int pmx_mgpu_gather_dev(pmx_mgpu *g, const uint64_t *const *d_shards, uint64_t *const *d_all, size_t n_total, size_t row_elems,
                        int root);
/* The LAST step of a job and its gather, overlapped: pmx_mgpu_permute_shards_dev in `chunks` pieces per shard (1 .. 16), piece i's
 * transfers - to rank `root`, or to every rank when root < 0 - posted on a second stream of each slot behind piece i's kernel, so
 * the links carry piece i while pieces i + 1 ... are computed.  To the streams of pmx_mgpu_stream the call is the permutation
 * followed by the gather (they wait for the transfers at the end).  d_all as above.  Only enqueues. */
int pmx_mgpu_permute_gather_dev(pmx_mgpu *g, uint64_t *const *d_shards, uint64_t *const *d_all, size_t n_total, int root, int chunks);
/* 2-to-1 Merkle tree of n_leaves = world * m leaves (both powers of two): d_nodes[local] = [2m-1][4] holds that rank's
 * m leaves in its first m rows and receives its subtree (pmx_merkle_2to1_dev); the `world` subtree roots are
 * all-gathered into d_top[local] = [2*world-1][4], which then receives the top levels, root last (world = 1: [1][4]).
 * Only enqueues. */
int pmx_mgpu_merkle_2to1_dev(pmx_mgpu *g, uint64_t *const *d_nodes, uint64_t *const *d_top, size_t n_leaves);
/* Host leaves [n_leaves][4] -> root [4] (single-process groups).  A host-buffer entry on every local device at once: it holds each
 * slot's context for the length of the call, as pmx_mgpu_permute_batch does, and its device staging (a subtree and the top levels per
 * slot) is kept by the group's contexts, grow-only, until the group is destroyed. */
int pmx_mgpu_merkle_2to1(pmx_mgpu *g, const uint64_t *leaves, size_t n_leaves, uint64_t *root);

/* (Test hooks of the device-group code - fault injection in the host fan-out, device groups whose slots share one GPU, a
 * named collective library - are declared in poseidon_mi355x_testing.h and exist only in libposeidon_mi355x_test.so, a
 * second build of the same objects; this library neither exports nor contains them.) */

/* (The benchmark diagnostics - the multiply-issue peak and the issue slot bench.py prices its kernels against - are NOT part of this
 * library: include/poseidon_mi355x_diag.h, libposeidon_mi355x_diag.so.) */

#ifdef __cplusplus
}
#endif
#endif /* POSEIDON_MI355X_H */
