// gm_probe.h — post-attach device validation for MI355X (gfx950), C ABI over HIP.
//
// The reference has no post-mount check at all: success means "mknod returned 0"
// (reference: pkg/util/util.go:64-70). gpumounter-amd proves an attached GPU is actually usable
// from the tenant side by running real CDNA4 kernels on it (wave64 liveness, HBM3E stream,
// MFMA bf16 peak and numerics) and, for multi-GPU attaches, by timing xGMI peer copies.
// All functions return hipError_t values (0 = success).
#pragma once
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gm_probe_props {
  char name[128];
  char gcn_arch[64];
  char pci_bus_id[32];   // "0000:05:00.0"
  int32_t cu_count;
  int32_t warp_size;
  uint64_t total_mem;
  uint64_t lds_per_block;
  int32_t clock_khz;
  int32_t mem_clock_khz;
} gm_probe_props_t;

int gm_probe_device_count(int* n);
int gm_probe_props(int dev, gm_probe_props_t* out);
// HIP device index whose PCI bus id matches `bdf` (case-insensitive "dddd:bb:dd.f"), -1 if none.
int gm_probe_find_device(const char* bdf, int* dev);
// Liveness: launches one wave64 kernel that writes lane ids and a checksum; verifies on host.
// *elapsed_us = launch→readback wall time.
int gm_probe_quick(int dev, int* ok, double* elapsed_us);
// What the liveness kernel writes and how the host judges it (one implementation, shared with the
// kernel: gm_quick_ref.h). With salt = 0x9e3779b9 ^ dev, all arithmetic in uint32:
//   word l, l = 0..63:  l · 2654435761 ^ salt        (lane l's own store)
//   word 64:            the sum of words 0..63        (64-lane shuffle reduction, lane 0 stores)
//   word 65:            64                            (popcount of the wave's ballot)
// The verdict makes three independent checks against that table and reports the ones that failed
// as bits: 1 a lane word, 2 the sum word, 4 the ballot word (GM_QUICK_BAD_*); 0 = healthy.
// Host only, no HIP call: the 66 expected words for `salt`; the verdict over a caller's 66 words.
// A null pointer is hipErrorInvalidValue.
int gm_probe_quick_expected(uint32_t salt, uint32_t* words);
int gm_probe_quick_verdict(const uint32_t* words, uint32_t salt, uint32_t* failed);
// Runs the kernel on `dev` exactly as gm_probe_quick does and returns the 66 raw words read back
// and the salt used, without judging them.
int gm_probe_quick_words(int dev, uint32_t* words, uint32_t* salt);
// gm_probe_quick's negative control: the same run, but word `word` (< 66) of the host copy is
// XORed with the nonzero `mask` before the verdict, so *ok must come out 0 and *failed must name
// that word's check. The device buffer and later runs are not affected. word >= 66, mask == 0 or
// a null pointer: hipErrorInvalidValue before any HIP call.
int gm_probe_quick_flip(int dev, uint32_t word, uint32_t mask, int* ok, uint32_t* failed,
                        double* elapsed_us);
// HBM3E stream: float4 copy of `bytes` for `iters`; *gbps = (read+write) bytes / time. The
// default variant is 2. Both timed drivers round `bytes` down to a multiple of 16 and return the
// HIP error of a failed launch instead of a rate.
int gm_probe_hbm_copy(int dev, uint64_t bytes, int iters, double* gbps);
// Read-only HBM stream over `bytes` (8 nontemporal 16-B loads in flight per lane); GB/s read.
int gm_probe_hbm_read(int dev, uint64_t bytes, int iters, int blocks_per_cu, double* gbps);
// Tuning variants: 0 grid-stride, 1 chunked 4×16B/lane, 2 chunked 4 + nontemporal,
// 3 chunked 8 + nontemporal, 4 chunked 8, 5/6 software-pipelined 4/2 (next loads before
// current stores), nontemporal. Any other variant is hipErrorInvalidValue.
int gm_probe_hbm_copy_variant(int dev, int variant, uint64_t bytes, int iters,
                              int blocks_per_cu, double* gbps);
// The launches the two timed drivers repeat, on caller-owned device buffers of the current
// device (`stream` may be NULL; asynchronous; the launch error is returned). Geometry: CUs ×
// blocks_per_cu blocks of 256 threads, each block a contiguous chunk of 16-byte elements rounded
// up to 1024 (copy) or 2048 (read) elements. Pointers 16-byte aligned, `bytes` a nonzero multiple
// of 16 (not rounded here), blocks_per_cu > 0, variant 0..6, src and dst disjoint: anything else
// is hipErrorInvalidValue before any HIP call.
// Exactly one launch of copy variant `variant`: dst[0, bytes) = src[0, bytes).
int gm_probe_copy(int variant, const void* src, void* dst, uint64_t bytes, int blocks_per_cu,
                  void* stream);
// Exactly one launch of the read stream. `sink` is 1024 uint32: every thread XORs the 32-bit
// words it reads (elements 256 apart in its block's chunk) and, only if that fold equals
// 0x9e3779b9, writes it to sink[b & 1023], b its block.
int gm_probe_read(const void* src, uint32_t* sink, uint64_t bytes, int blocks_per_cu,
                  void* stream);
// variant 0: v_mfma_f32_32x32x16_bf16 × 4 chains, 1: v_mfma_f32_16x16x32_bf16 × 4 chains,
// 2: 16x16x32 × 8 chains.
int gm_probe_mfma_peak_variant(int dev, int variant, int iters, int blocks_per_cu,
                               double* tflops);
// MFMA bf16 register-resident peak (best measured form: 16x16x32 × 8 chains); *tflops dense.
int gm_probe_mfma_peak(int dev, int iters, double* tflops);
// What those kernels compute: exactly one launch of peak kernel `variant` (0..2), through the
// launch the timed driver uses, with `blocks` blocks of 256 threads on the current device. The
// timed driver passes the kernel a null value pointer; here every thread stores every accumulator
// register after the loop: dev_out[block][thread][chain][register], chains × registers being
// 4 × 16 (variant 0), 4 × 4 (variant 1) and 8 × 4 (variant 2) floats per thread, so dev_out holds
// blocks × 256 × 64, 16 or 32 floats. Each wave of 64 threads computes, per chain, `iters`
// accumulations of one MFMA tile product C += A·B. With t = threadIdx.x, l = t & 63 and
// n_a(j), n_b(j) the integers below, lane l holds a[j] = bf16(seed · n_a(j)) and
// b[j] = bf16(seed · n_b(j)), j = 0..7 (product in fp32, then rounded to nearest even):
//   variant 0:    n_a = t + j,   n_b = j + 1;   A[l&31][8(l>>5)+j], B[8(l>>5)+j][l&31] (K = 16),
//                 register i of lane l is C[(i&3) + 8(i>>2) + 4(l>>5)][l&31]
//   variant 1, 2: n_a = 7t + j,  n_b = 3j + 1 + blockIdx.x;  A[l&15][8(l>>4)+j],
//                 B[8(l>>4)+j][l&15] (K = 32), register i of lane l is C[4(l>>4) + i][l&15]
// The chains take (A, B) from the lanes' (a, b), (b, a), (a, a), (b, b) in that order; variant 2
// repeats the four. Waits for the kernel. A variant outside 0..2, iters <= 0, blocks <= 0 or a
// dev_out that is null or not 16-byte aligned: hipErrorInvalidValue before any HIP call.
int gm_probe_mfma_peak_values(int variant, int iters, float seed, int blocks, float* dev_out,
                              void* stream);
// C[M,N] (fp32) = A[M,K] (bf16, row-major) · B[K,N] (bf16, row-major) on MFMA.
// Requires M%64 == 0, N%64 == 0, K%32 == 0 (checked). Device pointers; stream may be NULL.
int gm_probe_gemm_bf16(const void* A, const void* B, float* C, int M, int N, int K, void* stream);
// C[M,N] (bf16) = A[M,K] · Bt[N,K]ᵀ (bf16, both K-major), fp32 accumulate: the 256²-tile
// global_load_lds throughput GEMM. Requires M%256 == 0, N%256 == 0, K%64 == 0 (checked).
int gm_probe_gemm_nt(const void* A, const void* Bt, void* C, int M, int N, int K, void* stream);
// Schedule variants of the same kernel (A/B measurements; bench/gemm_sweep.py).
int gm_probe_gemm_nt_variant(int variant, const void* A, const void* Bt, void* C, int M, int N,
                             int K, void* stream);
// Dense bf16 TF/s of gm_probe_gemm_nt on uniform [-1,1] operands (gm_probe_fill_bf16), `iters`
// back-to-back launches.
int gm_probe_gemm_nt_tflops(int dev, int M, int N, int K, int iters, double* tflops);
// The operand fill of the two drivers below, on a caller-owned buffer of the current device:
// dst[i] = bf16(float(h >> 8) · 2/2^24 − 1), rounded to nearest even, with
//   h = (u32)i · 2654435761 ^ seed;  h ^= h >> 15;  h *= 2246822519;  h ^= h >> 13   (all u32).
// The values lie in [-1, 1]: the fp32 value is below 1, but the largest ones round to exactly
// 1.0 in bf16. The index is hashed as 32 bits, so the sequence repeats after 2^32 elements.
// `dst` 2-byte aligned, n_elems > 0 (checked); asynchronous on `stream` (may be NULL).
int gm_probe_fill_bf16(void* dst, uint64_t n_elems, uint32_t seed, void* stream);
// Number of 16-byte words that differ between a and b (the burn-in's compare kernel, with the
// burn-in's grid). Device pointers on the current device, both 16-byte aligned, `bytes` a nonzero
// multiple of 16 (checked before any HIP call); `stream` may be NULL; waits for the result.
int gm_probe_count_diff(const void* a, const void* b, uint64_t bytes, void* stream,
                        uint64_t* count);
// Burn-in: back-to-back n³ GEMMs (gm_probe_gemm_nt) for `seconds` on uniform [-1,1] operands;
// every result is compared bit-for-bit with the first (the kernel is deterministic), so
// *mismatches > 0 (16-B words that differ, summed over iterations) means silent data
// corruption. *tflops includes the compare kernels. n % 256 == 0.
int gm_probe_burn_in(int dev, int n, double seconds, double* tflops, uint64_t* mismatches,
                     int* iters);
// The burn-in's negative control (gm_probe_burn_in is its n_flips == 0 case): after the reference
// result is computed and before the loop starts, bf16 element flip_elems[i] (< n², all distinct)
// of the reference is XORed with the nonzero flip_masks[i] through a host round trip. The loop
// itself is unchanged, so *mismatches == *iters × (distinct 16-byte words among the flipped
// elements, i.e. distinct flip_elems[i] / 8). Bad flips: hipErrorInvalidValue before any HIP call.
int gm_probe_burn_in_flip(int dev, int n, double seconds, int n_flips,
                          const uint64_t* flip_elems, const uint16_t* flip_masks,
                          double* tflops, uint64_t* mismatches, int* iters);
// Self-contained numerics check of gm_probe_gemm_bf16 against a host fp32 reference.
int gm_probe_gemm_check(int dev, int M, int N, int K, double* max_abs_err, double* ref_scale);
// xGMI / PCIe peer copy a→b; *can_access from hipDeviceCanAccessPeer.
int gm_probe_p2p(int dev_a, int dev_b, uint64_t bytes, int iters, int* can_access, double* gbps);
const char* gm_probe_strerror(int err);

// ------------------------------------------------------------------ HBM pattern test (memtest)
// Free and total device memory of `dev` in bytes (hipMemGetInfo).
int gm_probe_mem_info(int dev, uint64_t* free_bytes, uint64_t* total_bytes);

// A test region is a logical range of bytes that may span several device allocations. Every
// 64-bit word of it has an expected value that is a pure function of (pattern, seed, pass, o),
// o = the word's global byte offset in the region (allocation base offset + local offset, a
// uint64_t multiple of 8), w = o / 8, all arithmetic modulo 2^64 (2^32 where marked u32):
//
//   GM_MEMTEST_ADDR    1   o ^ seed                      a word holds its own address
//   GM_MEMTEST_SOLID   2   0
//   GM_MEMTEST_CHECKER 4   0x5555555555555555
//   GM_MEMTEST_WALK    8   1 << ((w + pass) & 63)
//   GM_MEMTEST_RANDOM  16  v = w ^ seed ^ ((u64)(u32)(pass * 0x9E3779B9) << 32)
//                          x = (u32)v, y = (u32)(v >> 32)
//                          for c in 0x9E3779B9, 0x85EBCA6B, 0xC2B2AE35, 0x27D4EB2F:
//                            x = (u32)(rotl32(x, 24) + y) ^ c
//                            y = rotl32(y, 3) ^ x
//                          value = ((u64)y << 32) | x
//
// The inverted polarity of a pattern is the bitwise NOT of the value. The code is
// gm_memtest_pattern.h (shared by the host and the kernels).
typedef struct gm_memtest_record {
  uint64_t offset;    // global byte offset of the word in the region
  uint64_t expected;
  uint64_t got;
  uint32_t pattern;   // GM_MEMTEST_* bit
  uint32_t pass;
} gm_memtest_record_t;

#define GM_MEMTEST_MAX_RECORDS 16

typedef struct gm_memtest_result {
  uint64_t bytes_tested;
  uint64_t words_in_error;  // 64-bit words that differed, summed over every verify
  uint64_t bit_errors;      // sum of popcount(expected ^ got)
  uint64_t stuck_mask;      // OR of expected ^ got
  uint32_t records_filled;  // <= GM_MEMTEST_MAX_RECORDS; later mismatches are counted only
  uint32_t allocations;     // device allocations the driver used (0 for caller-owned buffers)
  gm_memtest_record_t records[GM_MEMTEST_MAX_RECORDS];
  double seconds;           // wall time of the whole call
  double write_gbps;        // bytes written by the fill kernels / their time
  double read_gbps;         // bytes read by the verify-only kernels / their time
  double rw_gbps;           // bytes read + written by verify-and-invert / its time
} gm_memtest_result_t;

// Host-side evaluation of the pattern function: out[i] = value of the word at byte offset
// base_offset + 8 i. Needs no GPU. base_offset % 8 == 0, pattern one GM_MEMTEST_* bit.
int gm_probe_memtest_expected(uint32_t pattern, uint64_t seed, uint32_t pass,
                              uint64_t base_offset, uint64_t n_words, uint64_t* out);
// Fill / check a caller-owned device buffer on the current device. `ptr` 16-byte aligned,
// `bytes` a nonzero multiple of 16, `base_offset` a multiple of 8, `pattern` one GM_MEMTEST_*
// bit: anything else is hipErrorInvalidValue before any HIP call. `invert` selects ~P.
// Both are asynchronous on `stream` (may be NULL) except that verify waits for its result.
int gm_probe_memtest_fill(void* ptr, uint64_t bytes, uint32_t pattern, int invert, uint64_t seed,
                          uint32_t pass, uint64_t base_offset, void* stream);
// With `write_inverse` the same kernel also writes the opposite polarity over every word it has
// read (whatever it read there). Only the error fields and bytes_tested of *out are set.
int gm_probe_memtest_verify(void* ptr, uint64_t bytes, uint32_t pattern, int invert,
                            int write_inverse, uint64_t seed, uint32_t pass,
                            uint64_t base_offset, void* stream, gm_memtest_result_t* out);
// The self-contained test of `bytes` (multiple of 16) of device memory on `dev`, allocated in
// pieces of at most `chunk_bytes` (0 = 8 GiB, else a multiple of 16). For each pattern of
// `pattern_mask` and each of `passes`: fill(P), verify P while writing ~P, verify ~P, every kernel
// over the whole region in the same order. A failed allocation is retried at half the size (not
// below min(256 MiB, its size)); if that fails too, the test runs on what it has and
// out->bytes_tested says how much; the HIP error is returned only if nothing could be allocated.
// flip_mask != 0 is the negative control: after every fill(P) the word at global byte offset
// flip_offset (multiple of 8, inside `bytes`) is XORed with flip_mask through a host round trip;
// it is skipped if the offset lies beyond what could be allocated.
int gm_probe_memtest(int dev, uint64_t bytes, uint64_t chunk_bytes, uint32_t pattern_mask,
                     int passes, uint64_t seed, uint64_t flip_offset, uint64_t flip_mask,
                     gm_memtest_result_t* out);
// Tuning hook: 1 = nontemporal stores in fill and verify-and-invert (default), 0 = plain stores.
// Returns the previous setting; any other value only queries.
int gm_probe_memtest_store_variant(int nontemporal);

// ------------------------------------------------------------------ per-CU self-test (CU scan)
// One kernel runs the selected tests in a 256-thread block (4 waves) that statically declares the
// whole 160 KiB of LDS, so at most one block is resident per CU and a grid of cu_count blocks on
// an idle device can cover every CU. HIP promises nothing about placement: where a block ran is
// read from the hardware registers and only *observed*; no result depends on it.
//
// CU id (12 bits) = XCC_ID[3:0] << 8 | HW_ID[15:8]; HW_ID[15:8] is CU_ID 11:8, SH_ID 12,
// SE_ID 15:13 (2 bits on gfx942/950, the top bit reads 0); a wave's SIMD is HW_ID[5:4]. The id is
// an attribution label taken from the registers, not something a result depends on.
//
// Every test gives 4 uint32 words per thread t (0..255), 1024 per block: word 4 t + i. They are a
// pure function of (test, seed, iters, t), never of the block or its placement; the expected
// table is computed on the host, uploaded once per scan and compared in the kernel. All integer
// arithmetic is modulo 2^32. The code is gm_cuscan_sig.h (shared by the host and the kernel).
//
//   H(test, idx):  h = (u32)seed ^ (idx * 0x9E3779B1)
//                  h ^= h >> 16;  h *= 0x85EBCA6B;  h ^= h >> 13
//                  h += (u32)(seed >> 32) ^ (test * 0xC2B2AE35)
//                  h ^= h >> 16;  h *= 0xC2B2AE35;  h ^= h >> 13;  h *= 0x27D4EB2F;  h ^= h >> 16
//
//   GM_CUSCAN_VALU_INT 1   two chains (x0, y0), (x1, y1) = H(1, 4t), H(1, 4t+1), H(1, 4t+2),
//                          H(1, 4t+3); for s in 0 .. 128 iters - 1, on both chains, with
//                          k = (0x9E3779B9, 0x85EBCA6B, 0xC2B2AE35, 0x27D4EB2F)[s & 3]:
//                            x = (rotl32(x, 24) + y) ^ k;   y = rotl32(y, 3) ^ x
//                            m = (u64)x * (y | 1);   x ^= (u32)(m >> 32);   y += (u32)m
//                          words x0, y0, x1, y1
//   GM_CUSCAN_VALU_F32 2   four fp32 chains j = 0..3 with h1 = H(2, 4t+j), h2 = H(2, 1024+4t+j):
//                            x = 1 + (h1 >> 9) / 2^23,  a = 1 + (h2 >> 20) / 2^12,
//                            b = (h2 & 0xFFFFFF) / 2^24
//                          for 64 iters steps: x = fmaf(x, a, b);  x = x - floorf(x) + 1
//                          x * a + b needs fewer than 53 bits, so float32(float64(x) * a + b) is
//                          the correctly rounded FMA; the range reduction is exact. Word j is the
//                          bit pattern of chain j.
//   GM_CUSCAN_MFMA     4   per wave w = t / 64: C_w = sum over s in 0 .. 4 iters - 1 of
//                          A_{w,s} (16x32) . B_{w,s} (32x16) with v_mfma_f32_16x16x32_bf16, where
//                            A[r][k] = E(H(4, ((4s + w) * 2 + 0) * 64 + r + 16 (k >> 3)), k & 7)
//                            B[k][c] = E(H(4, ((4s + w) * 2 + 1) * 64 + c + 16 (k >> 3)), k & 7)
//                            E(h, j) = ((h >> 4j) & 15) % 9 - 4           an integer in [-4, 4]
//                          Every product and partial sum is an exact fp32 integer in any order
//                          as long as 32 * 16 * steps < 2^24: iters <= 8191 (checked). Word i of
//                          lane l = t % 64 is the fp32 bit pattern of C_w[4 (l >> 4) + i][l & 15],
//                          the instruction's own accumulator layout.
//   GM_CUSCAN_LDS      8   march over all 40960 words of the block's LDS, iters rounds r with
//                          P(a) = H(8, 65536 r + a), s0 = s1 = s2 = s3 = 0 before the first:
//                           1. thread t writes P to the 16-byte elements v = 256 k + t, k < 40
//                              (words 4v .. 4v+3) with 128-bit stores; barrier
//                           2. for i < 160: a = ((256 i + t) * 12347 + 7) % 40960 (a permutation
//                              of the addresses: the stride is odd and no multiple of 5), 32-bit
//                              read g of word a; s0 = rotl32(s0, 5) + g; s3 += (g != P(a));
//                              32-bit write of ~g to word a; barrier
//                           3. for k < 40: 128-bit read of element v = 256 k + (t + 64) % 256, and
//                              for each of its words g, c = 0..3: s1 = rotl32(s1, 7) ^ g;
//                              s2 += g; s3 += (g != ~P(4v + c)); barrier
//                          words s0, s1, s2, s3 (s3 = mismatches seen in flight, expected 0).
//                          Every word is written and read in both polarities. The element read
//                          in phase 3 was first written by the next wave; of the permuted reads
//                          of phase 2 about three in four are of a word another wave wrote.
//
// What the scan cannot see: clocks and thermals (the transcendental units, register-file
// addressing, the scalar unit and the cross-lane network are the lane scan's, the vector L1, L2,
// scalar and instruction caches the cache scan's, both below).
// The GM_CUSCAN_* test bits and the iters limits are defined in gm_cuscan_sig.h.
#define GM_CUSCAN_MAX_RECORDS 16
#define GM_CUSCAN_IDS 4096
#define GM_CUSCAN_ANY 0xFFFFFFFFu

typedef struct gm_cuscan_record {
  uint32_t id;        // CU id the block ran on
  uint32_t simd;      // SIMD of the wave that computed the word
  uint32_t test;      // GM_CUSCAN_* bit
  uint32_t thread;    // 0..255
  uint32_t word;      // 0..3
  uint32_t expected;
  uint32_t got;
  uint32_t pad;
} gm_cuscan_record_t;

// Negative control, a data flip: in every block that runs on a CU whose id is `id` (any CU with
// GM_CUSCAN_ANY), `mask` (nonzero) is XORed into word `word` of thread `thread` of `test`'s
// computed signature before the compare.
typedef struct gm_cuscan_inject {
  uint32_t id, test, thread, word, mask;
} gm_cuscan_inject_t;

typedef struct gm_cuscan_cu {
  uint32_t id, xcc, se, sh, cu;
  uint32_t runs;          // blocks that ran here
  uint32_t failed_runs;   // of which had a wrong word
  uint32_t tests_failed;  // mask of GM_CUSCAN_* bits
  uint32_t simds_seen;    // mask of the SIMDs that waves of those blocks ran on
  uint32_t simds_failed;  // mask of the SIMDs whose wave had a wrong word
} gm_cuscan_cu_t;

typedef struct gm_cuscan_result {
  uint32_t cus_expected;    // multiProcessorCount
  uint32_t cus_seen;        // distinct ids; > cus_expected would mean the id holds a bit that is
                            // not a location: reported, never hidden
  uint32_t complete;        // cus_seen == cus_expected
  uint32_t rounds;
  uint64_t blocks_run;
  uint64_t words_in_error;
  uint64_t blocks_four_simds;  // blocks whose four waves reported four distinct SIMDs
  uint32_t failed_cus;
  uint32_t records_filled;  // <= GM_CUSCAN_MAX_RECORDS; later wrong words are counted only
  uint32_t xcc_cus[16];     // distinct ids per XCC
  gm_cuscan_record_t records[GM_CUSCAN_MAX_RECORDS];
  double seconds;           // wall time of the whole call
  double kernel_ms;         // the rounds' kernels alone, summed (event pairs)
} gm_cuscan_result_t;

// out[4 t + i] = word i of thread t. Host only, needs no GPU. `test` one GM_CUSCAN_* bit,
// 1 <= iters <= GM_CUSCAN_MAX_ITERS (GM_CUSCAN_MFMA_MAX_ITERS for the MFMA test).
int gm_probe_cuscan_expected(uint32_t test, uint64_t seed, uint32_t iters, uint32_t* out);
// Exactly one block of the scan's device code on the current device, which writes the raw
// signature of `test` to dev_out (1024 uint32, 16-byte aligned) instead of comparing it, and to
// dev_where (5 uint32) the CU id, then the four waves' SIMD ids. Asynchronous on `stream`.
int gm_probe_cuscan_signature(uint32_t test, uint64_t seed, uint32_t iters, uint32_t* dev_out,
                              uint32_t* dev_where, void* stream);
// The scan of device `dev`. A round is one launch of cu_count blocks followed by a read of the
// distinct-id counter; the scan stops after min_rounds once every CU has been seen, or at
// max_rounds (1 <= min_rounds <= max_rounds <= 1024). `cus` (cus_cap entries, may be NULL with
// cus_cap 0) receives one entry per CU seen, sorted by id; *n_cus (may be NULL) how many there are,
// which may exceed cus_cap. Bad arguments, among them an injection whose test is not in
// tests_mask: hipErrorInvalidValue before any HIP call.
int gm_probe_cuscan(int dev, uint32_t tests_mask, uint32_t iters, uint64_t seed, int min_rounds,
                    int max_rounds, const gm_cuscan_inject_t* inject, gm_cuscan_result_t* out,
                    gm_cuscan_cu_t* cus, int cus_cap, int* n_cus);

// ------------------------------------------------------------------ matrix-core format scan
// The CU scan's frame (one 256-thread block per CU, the whole LDS declared, the CU id read from
// the registers, a host-computed table compared bit for bit) around the matrix cores in the
// formats the CU scan's bf16 test leaves out. Every wave w = t / 64 runs `iters` dependent MFMAs
// of each selected format; word i of lane l = t % 64 is the bit pattern of accumulator register i
// (f64: lo ^ rotl32(hi, 16); i8: the int32). The code is gm_mfmascan_ref.h (shared by the host
// and the kernel). H is the CU scan's hash; format index f = log2(bit).
//
//   bit   name   instruction                                         K    elements per lane
//      1  f16    v_mfma_f32_16x16x32_f16                              32    8 half words
//      2  fp8    v_mfma_f32_16x16x32_fp8_fp8 (OCP e4m3)               32    8 bytes
//      4  bf8    v_mfma_f32_16x16x32_bf8_bf8 (e5m2)                   32    8 bytes
//      8  i8     v_mfma_i32_16x16x64_i8                               64   16 bytes
//     16  f32    v_mfma_f32_16x16x4_f32                                4    1
//     32  f64    v_mfma_f64_16x16x4_f64                                4    1
//     64  mxfp8  v_mfma_scale_f32_16x16x128_f8f6f4, cbsz = blgp = 0  128   32 bytes     (e4m3)
//    128  mxbf8  the same, 1                                         128   32 bytes     (e5m2)
//    256  mxfp6  the same, 2                                         128   32 x 6 bits  (e2m3)
//    512  mxbf6  the same, 3                                         128   32 x 6 bits  (e3m2)
//   1024  mxfp4  the same, 4                                         128   32 nibbles   (e2m1)
//
// Operands. Lane l's operand m (0: A, 1: B) in step s is built from the hash words
//   h_q = H(0x200 + f, ((((4 s + w) * 2 + m) * 64 + l) * 4 + q),  q = 0..3
// Nibble formats (f16, fp8, bf8, mx*): element e is nibble n = (h_{e >> 3} >> 4 (e & 7)) & 15 and
// stands for the e2m1 value of n: magnitude (0, 1/2, 1, 3/2, 2, 3, 4, 6)[n & 7], negative when
// n & 8 (so -0 occurs). The format's 16-entry code table encodes it: all 16 values are exact in
// f16, e4m3, e5m2, e2m3 and e3m2; for mxfp4 the register image is h_0..h_3 itself. Packing:
// 16-, 8- and 4-bit codes in element order from the low end of the lane's registers; 6-bit codes
// as bits [6 e, 6 e + 6) of the 192-bit little-endian string of registers 0..5.
//   i8:  the 16 bytes of h_0..h_3, signed, full range.
//   f32: h_0 % 511 - 255;   f64: (h_0 & (2^23 - 1)) - 2^22.
// mx* scales: the E8M0 byte of A's row i is 127 + (H(0x220 + f, (2 w + 0) * 16 + i) & 3) - 2, of
// B's column j the same with (2 w + 1) * 16 + j: constant over the steps, the same in all four
// lanes that hold the row (i, i + 16, i + 32, i + 48), byte 0 of the scale register, opsel 0.
//
// Expected value, over register images (a(l, e) = element e of lane l's A image):
//   C[i][j] = sum over s < iters, h < 4, e of a_s(i + 16 h, e) * b_s(j + 16 h, e)
//             (mx*: times 2^(sA_i + sB_j - 254))
// and lane l register r holds C[4 (l >> 4) + r][l & 15] (f64: C[(l >> 4) + 4 r][l & 15]). This
// rests on: lane l carries row / column l & 15 and K-group l >> 4; element e of a K-group names
// the same k in A and in B; the C/D map above.
//
// Exactness: in quarter units a nibble product is at most 144, so 144 * K * iters < 2^24 keeps
// every partial sum an exact fp32 in any order (iters <= 910 at K = 128), and the power-of-two
// scale only moves the exponent. i8: 2^14 * 64 * iters < 2^31. f32: 4 * 255^2 * iters < 2^24
// (iters <= 63). f64: 4 * 2^44 * iters < 2^53. One limit for all: GM_MFMASCAN_MAX_ITERS = 63
// (static_asserts in gm_mfmascan_ref.h). A sum of zero is +0.0.
//
// Not covered: the dense 32x32 shapes and mixed A/B formats of v_mfma_* (the sparse scan below
// covers v_smfmac_*, its 32x32 forms and its two mixed fp8/bf8 forms), a different scale per
// K-block of a row, NaN / infinity / subnormal operands, rounding (nothing here rounds).
//
// The records, the injection, the per-CU entries and the result are the CU scan's, with `test`
// and `tests_failed` holding GM_MFMASCAN_* format bits. Arguments and the up-front
// hipErrorInvalidValue checks are those of the gm_probe_cuscan* counterparts, with
// 1 <= iters <= GM_MFMASCAN_MAX_ITERS.
int gm_probe_mfmascan_expected(uint32_t format, uint64_t seed, uint32_t iters, uint32_t* out);
// The operand register images the kernel feeds the instruction in step `step` (<
// GM_MFMASCAN_MAX_ITERS): images[((w * 2 + m) * 64 + l) * 8 + d] = dword d of lane l's operand m
// in wave w (4096 words), and scales[(w * 2 + m) * 16 + r] the E8M0 byte of row / column r (128
// words; 127 for a format without scales). Host only, needs no GPU.
int gm_probe_mfmascan_images(uint32_t format, uint64_t seed, uint32_t step, uint32_t* images,
                             uint32_t* scales);
int gm_probe_mfmascan_signature(uint32_t format, uint64_t seed, uint32_t iters, uint32_t* dev_out,
                                uint32_t* dev_where, void* stream);
int gm_probe_mfmascan(int dev, uint32_t formats_mask, uint32_t iters, uint64_t seed,
                      int min_rounds, int max_rounds, const gm_cuscan_inject_t* inject,
                      gm_cuscan_result_t* out, gm_cuscan_cu_t* cus, int cus_cap, int* n_cus);

// ------------------------------------------------------------------ sparse and 32x32 scan
// The same frame around the sparse matrix path, v_smfmac_*: a datapath of its own with an index
// register, a 4:2 operand selector in front of the multipliers and an `abid` set selector; half
// of its forms have the 32x32 C/D layout (16 accumulator registers per lane) and two take A and
// B in different 8-bit formats. Every wave w = t / 64 runs `iters` dependent SMFMACs of each
// selected form. The code is gm_sparsescan_ref.h (shared by the host and the kernel,
// native/hip/gm_sparsescan.hip). Format index f = log2(bit).
//
//   bit   name        instruction                                       dense K  A kept / B dense
//      1  f16         v_smfmac_f32_16x16x64_f16                            64     8 / 16 half words
//      2  bf16        v_smfmac_f32_16x16x64_bf16                           64     8 / 16 half words
//      4  i8          v_smfmac_i32_16x16x128_i8                           128    16 / 32 bytes
//      8  fp8         v_smfmac_f32_16x16x128_fp8_fp8 (OCP e4m3)           128    16 / 32 bytes
//     16  bf8         v_smfmac_f32_16x16x128_bf8_bf8 (e5m2)               128    16 / 32 bytes
//     32  fp8bf8      v_smfmac_f32_16x16x128_fp8_bf8 (A e4m3, B e5m2)     128    16 / 32 bytes
//     64  bf8fp8      v_smfmac_f32_16x16x128_bf8_fp8 (A e5m2, B e4m3)     128    16 / 32 bytes
//    128  f16-32x32   v_smfmac_f32_32x32x32_f16                            32     8 / 16 half words
//    256  bf16-32x32  v_smfmac_f32_32x32x32_bf16                           32     8 / 16 half words
//    512  i8-32x32    v_smfmac_i32_32x32x64_i8                             64    16 / 32 bytes
//   1024  fp8-32x32   v_smfmac_f32_32x32x64_fp8_fp8                        64    16 / 32 bytes
// Per lane A is 4 registers of kept elements, B 8 registers of dense ones, and there is one index
// register; cbsz is 0.
//
// The model. These are premises: what the scan's table rests on, each checked on the hardware
// through gm_probe_sparsescan_apply with operands the caller builds (profiles/sparsescan/README.md
// says what a run found).
//  1. Dense group to kept pair. A is 2:4 compressed. Dense group g of a lane is the four
//     consecutive K positions 4 g .. 4 g + 3 of the lane's K-group; the lane's kept elements 2 g
//     and 2 g + 1 belong to it.
//  2. Index word. Bits [4 g, 4 g + 2) and [4 g + 2, 4 g + 4) of the lane's index set are the
//     positions i0 and i1 (0..3): kept element 2 g + p multiplies B's dense element 4 g + i_p of
//     the paired lane. A 16-bit form has 4 groups per lane, a set is 16 bits and the register
//     holds two: with cbsz 0, abid 0 / 1 selects the low / high half. An 8-bit form has 8 groups:
//     the set is the whole register and abid stays 0.
//  3. Lane maps. 16x16: lane l carries row (A) / column (B) l & 15 and K-group h = l >> 4 (four
//     K-groups). 32x32: row / column l & 31, K-group h = l >> 5 (two). With D dense elements per
//     lane (16 or 32) and K = D * K-groups, dense element e of A's expansion is k = D h + e, and
//     element e of B is k = (K / 2) (e / (D / 2)) + (D / 2) h + e % (D / 2): B is laid out as two
//     instructions of half the K side by side, A's expansion is contiguous. (The premise this
//     started from, "element e of a K-group names the same k in A's dense expansion and in B",
//     was wrong on the hardware in every form; one-hot operands through gm_probe_sparsescan_apply
//     gave the map above.) C/D 16x16: register r of lane l is row 4 (l >> 4) + r, column l & 15.
//     C/D 32x32: register r of 16 is row 8 (r >> 2) + 4 (l >> 5) + (r & 3), column l & 31.
//
// Operands. H is the CU scan's hash. Lane l's operand m (0: A, 1: B) in step s is built from
//   h_q = H(0x700 + f, ((((4 s + w) * 2 + m) * 64 + l) * 8 + q),  q = 0..7
// Element e is nibble (h_{e >> 3} >> 4 (e & 7)) & 15, the e2m1 value of the format scan, coded by
// the operand's table (f16, e4m3, e5m2 as there; bf16: the upper half word of the value's fp32
// pattern) and packed in element order from the low end of the registers. i8: A is the 16 bytes
// of h_0..h_3, B the 32 bytes of h_0..h_7, signed, full range.
// Index register: nibble j = pair(H(0x720 + f, ((4 s + w) * 64 + l) * 8 + j) % 6), pair(p) =
// i0 | i1 << 2 of the p-th of (0,1) (0,2) (0,3) (1,2) (1,3) (2,3). An 8-bit form's nibble j is
// group j; a 16-bit form's is group j & 3 of set j >> 2, both sets filled independently, and step
// s runs with abid = s & 1 (two call sites: abid is an immediate).
//
// Expected value, over register images: dense_a(l, 4 g + i_p) = a(l, 2 g + p), zero elsewhere;
//   A_s[l % R][D (l / R) + e] = dense_a_s(l, e),  B_s[k of premise 3][l % R] = b_s(l, e),
//   C[i][j] = sum over s < iters, k < K of A_s[i][k] * B_s[k][j]
// with R = 16 and 4 K-groups or R = 32 and 2. Word i of a 16x16 form's signature is the bit
// pattern of accumulator register i; of a 32x32 form's the fold of registers 4 i .. 4 i + 3,
// x = rotl32(x, 5) + bits from 0, so that a wrong word still names a band of rows.
//
// Exactness: in quarter units a nibble product is at most 144 and an output sums at most 64 kept
// products per step: 144 * 64 * iters < 2^24. i8: 2^14 * 64 * iters < 2^31. One limit,
// GM_SPARSESCAN_MAX_ITERS = 63 (static_asserts in gm_sparsescan_ref.h). A sum of zero is +0.0.
//
// Cannot tell: index pairs with i0 >= i1 are never issued (what the hardware does with them is
// not documented here); cbsz != 0 and the broadcast it selects; abid with an 8-bit form; the
// dense 32x32 v_mfma_* instructions; NaN / infinity / subnormal operands and rounding (nothing
// here rounds); which of a lane's two kept elements of a group a product used when both B
// elements and both kept elements are equal.
//
// The records, the injection, the per-CU entries and the result are the CU scan's, with `test`
// and `tests_failed` holding GM_SPARSESCAN_* format bits. Arguments and the up-front
// hipErrorInvalidValue checks are those of the gm_probe_mfmascan* counterparts.
int gm_probe_sparsescan_expected(uint32_t format, uint64_t seed, uint32_t iters, uint32_t* out);
int gm_probe_sparsescan_signature(uint32_t format, uint64_t seed, uint32_t iters,
                                  uint32_t* dev_out, uint32_t* dev_where, void* stream);
int gm_probe_sparsescan(int dev, uint32_t formats_mask, uint32_t iters, uint64_t seed,
                        int min_rounds, int max_rounds, const gm_cuscan_inject_t* inject,
                        gm_cuscan_result_t* out, gm_cuscan_cu_t* cus, int cus_cap, int* n_cus);
// The register images the kernel feeds the instruction in step `step` (< GM_SPARSESCAN_MAX_ITERS):
// a[(w * 64 + l) * 4 + d] (1024 words), b[(w * 64 + l) * 8 + d] (2048), idx[w * 64 + l] (256) and
// *abid, that step's set selector. Host only, needs no GPU.
int gm_probe_sparsescan_images(uint32_t format, uint64_t seed, uint32_t step, uint32_t* a,
                               uint32_t* b, uint32_t* idx, uint32_t* abid);
// One block, one instruction of `format` per wave on images the caller built (laid out as
// gm_probe_sparsescan_images gives them, in device memory, a / b / out 16-byte aligned), from a
// zero accumulator: dev_out[16 t + r] = the bit pattern of accumulator register r of thread t; a
// 16x16 form fills r < 4 and zeroes the rest. abid: 0 or 1, 1 only for a 16-bit form. Bad
// arguments: hipErrorInvalidValue before any HIP call.
int gm_probe_sparsescan_apply(uint32_t format, uint32_t abid, const uint32_t* dev_a,
                              const uint32_t* dev_b, const uint32_t* dev_idx, uint32_t* dev_out,
                              void* stream);

// ------------------------------------------------------------------ MX GEMM burn-in
// The burn-in's second load: a GEMM on the block-scaled matrix pipe
// (v_mfma_scale_f32_16x16x128_f8f6f4), HBM → LDS → MFMA → HBM like the bf16 one, every result
// compared bit for bit with the first. The code is gm_mxgemm_ref.h (shared by the host and the
// fill kernel) and native/hip/gm_mxgemm.hip.
//
// Formats (`fmt` is the instruction's format field): 0 = mxfp8, OCP e4m3 (bias 7, subnormals, no
// infinities, 0x7f / 0xff NaN); 4 = mxfp4, e2m1 (nibble n: magnitude (0, 1/2, 1, 3/2, 2, 3, 4, 6)
// [n & 7], negative when n & 8).
//
// Operands. A[M][K] and Bt[N][K] are K-major and packed: fp8 one byte per element; fp4 two
// elements per byte, element 2 i in the low nibble of byte i. Scales sA[M][K/32], sB[N][K/32]:
// one E8M0 byte per row and 32 elements of K, row-major, 127 = 1.0. C[M][N] is bf16:
//   C[i][j] = bf16( sum over k of a(i,k) * 2^(sA[i][k/32] - 127) * b(j,k) * 2^(sB[j][k/32] - 127) )
// summed in fp32 by the matrix core, rounded to nearest even at the end.
//
// Fill. With h(i, s) = the hash of gm_probe_fill_bf16 ((u32)i * 2654435761 ^ s; h ^= h >> 15;
// h *= 2246822519; h ^= h >> 13), element e = row * K + k of an operand with seed `seed` has
// H = h(e, seed) and the code
//   class 0 exact    nibble n = H >> 28; fp4: n itself; fp8: the e4m3 code of n's e2m1 value
//                    (the matrix-core scan's table: magnitudes 00 30 38 3c 40 44 48 4c, sign 0x80)
//   class 1 blocks   nibble (0, 2, 4, 10, 12)[(H >> 8) % 5], i.e. 0, 1, 2, -1, -2; coded as above
//   class 2 random   fp4: nibble H >> 28. fp8: byte b = H >> 24, and where (b & 0x7f) == 0x7f
//                    (a NaN code) b = (b & 0x80) | ((H >> 8) & 0x7e) instead
// and the scale byte of (row, K-block kb), with S = seed ^ 0x5ca1e5ca and kblocks = K / 32:
//   exact    125 + (h(row, S) >> 30)                    125..128, the same along K
//   blocks   127 + (h(row * kblocks + kb, S) >> 31)     127 or 128, different along K
//   random   123 + (h(row * kblocks + kb, S) >> 29)     123..130
// Indices are hashed as 32 bits. A and Bt are filled with different seeds.
//
// What each class checks. exact: every product is a multiple of 2^-2 * 2^(sA + sB - 254) and at
// most 144 of them, all products of one output share one scale, so the sum is exact in fp32 in
// any order while 144 * K < 2^24 (in units of 2^-6, the smallest scale: 9216 * K < 2^24). blocks:
// scaled operands are 0, ±1, ±2, ±4, products integers of at most 16 in magnitude, a 128-term sum
// at most 2048: exact in any order, and a scale applied to the wrong k changes the result, which
// `exact` cannot see. random: the load; no NaN code, |scaled value| <= 448 * 8, so no infinity at
// any K an int can hold. The result rounds, so it is checked against the float64 sum `ref` with
// the bound |C - ref| <= 2^-9 * sum|product| + 2^-8 * |ref|.
//
// Fills `rows` rows of K elements (K % 32 == 0) and their rows * K/32 scale bytes, on the current
// device, asynchronous on `stream`. Bad arguments: hipErrorInvalidValue before any HIP call.
int gm_probe_mx_fill(int fmt, int cls, uint32_t seed, int rows, int K, void* elems, void* scales,
                     void* stream);
// The GEMM on device pointers: 256×256 tiles, a K-tile of 128 bytes per row. M % 256 == 0,
// N % 256 == 0, K % 128 == 0 (fp8) or K % 256 == 0 (fp4), A and Bt 16-byte, sA and sB 4-byte,
// C 2-byte aligned: checked before any HIP call. Asynchronous on `stream` (may be NULL).
int gm_probe_mxgemm_nt(int fmt, const void* A, const void* sA, const void* Bt, const void* sB,
                       void* C, int M, int N, int K, void* stream);
// Host only, no GPU: the expected result for operands filled with (fmt, cls, seed_a) and
// (fmt, cls, seed_b), any M, N > 0 and K % 32 == 0. exact, blocks: c[i * N + j] = the bf16 bits of
// the exact integer sum (ref, abs_sum unused, may be NULL). random: ref[i * N + j] = the float64
// sum in k order and abs_sum[i * N + j] = the sum of |product| (c unused, may be NULL).
int gm_probe_mxgemm_expected(int fmt, int cls, uint32_t seed_a, uint32_t seed_b, int M, int N,
                             int K, uint16_t* c, double* ref, double* abs_sum);
// Registers and scratch bytes of the format's kernel (the accumulators must stay in registers).
int gm_probe_mxgemm_kernel_info(int fmt, int* num_regs, int* scratch_bytes);
// The MX burn-in: gm_probe_burn_in_flip's contract and loop with gm_probe_mxgemm_nt on
// random-class n × n operands (seeds 0x5151, 0xa3a3) as the GEMM. n % 256 == 0; the flips are
// bf16 elements of the n × n reference; *mismatches == *iters × (distinct 16-byte words among the
// flipped elements); *tflops counts 2 n³ per GEMM, compare kernels included.
int gm_probe_mx_burn_in_flip(int dev, int fmt, int n, double seconds, int n_flips,
                             const uint64_t* flip_elems, const uint16_t* flip_masks,
                             double* tflops, uint64_t* mismatches, int* iters);

// ------------------------------------------------------------------ attributed burn-in
// The burn-ins above compare the GPU with itself through a fixed block → tile map, so a tile is
// recomputed where the reference computed it, and a mismatch names no unit. The attributed
// burn-in is the same load with the map rotated from one iteration to the next: a tile's bits
// depend on its operands and the kernel's summation order, not on the block that computes it,
// so block b may compute the tile the plain map gives block (b + r) mod grid, for any r. Every
// block stores the 12-bit id of the CU it ran on (the scans' id: XCC_ID << 8 | HW_ID[15:8]) under
// its tile, and a per-tile compare turns a mismatch into an event between two known CUs. The
// code shared by host and device (the map, the step, the blame rule) is gm_burnin_attr.h.
//
// The loop, on the null stream, in order:
//   warm-up    one whole iteration outside the timing: a traced GEMM at r = 0 without the
//              injection, and the compare of its result with itself; `first` = the CU of its
//              tile 0, which the later kernels read on the device
//   reference  one traced GEMM at r = 0 into the reference and the same compare; its CU map is
//              kept; the flips are applied to it exactly as gm_probe_burn_in_flip applies them
//              From the warm-up on the stream holds GEMM, compare, GEMM, compare ... with no
//              host round trip in between (the flips' copies apart). On the one MI355X this was
//              measured on, where the blocks of a launch run depends on the launches before it
//              and repeats with a short period, so a warm-up that is one more turn of the
//              loop's own sequence makes `first` a CU the loop comes back to. That is observed,
//              not promised.
//   iteration i = 1, 2, ...  a traced GEMM at r = (i · step) mod grid, then the per-tile compare.
//              grid = (n / 256)² blocks = tiles; step is coprime to grid and, where grid > 8, no
//              multiple of 8 (gm_burnin_step), so a tile changes XCD from one iteration to the
//              next and meets every block within grid iterations.
// The compare (one block per tile) counts the tile's differing 16-byte words, the unit and the
// total of the plain burn-in's compare. A tile with none whose CU differs from the reference's is
// marked exonerated: another CU reproduced the reference's bits. A tile with some adds them to
// *mismatches and appends an event to a log of GM_BURNIN_LOG_CAP entries; later events are
// counted (events) but not logged (log_overflow). Every tile also marks its CU in `seen` and,
// where its CU differs from the reference's, itself in `moved`. An id of GM_CUSCAN_IDS or more
// in either map is no CU's (0xFFFFFFFF: the block stored nothing): such a tile marks nothing
// in `seen`, and its event is logged with the ids as read.
//
// The blame, decided on the host after the loop (exoneration may come after the event): an
// event at tile t with worker W and reference R blames W if t is exonerated or W == R, else R.
// A tile no other CU ever reproduced makes the reference the odd one out. W is blamed in the
// role of the worker, R in the role of the reference. W == R (in a grid of g blocks every g-th
// iteration runs at r = 0, where a block may land on the reference's CU again) counts as the
// worker's, except at a tile that is not exonerated and at which another CU disagreed with the
// reference in a logged event too: the reference is then the odd one out for its own CU as for
// the others, and the event counts as the reference's. Under log_overflow
// only the logged events are blamed. A logged event with an id that is no CU's blames nobody,
// so a run that holds one gives no verdict: the burn-in returns hipErrorUnknown, as it does when
// the warm-up's tile 0 stored no id.
//
// The injection is the negative control that the flips cannot be: a CU that is consistently
// wrong, in the reference too. Every block that finds itself on CU `id` XORs `mask` into the
// bf16 element (0, 0) of its tile on the way out. first != 0: the id is taken from the warm-up
// (the CU that computed tile 0) and `id` is ignored.
#define GM_BURNIN_LOG_CAP 1024
#define GM_BURNIN_MAX_RECORDS 16

typedef struct gm_burnin_event {
  uint32_t iteration;  // 1-based
  uint32_t tile;       // row-major over the (n / 256)² tiles
  uint32_t worker;     // CU id of the block that computed the mismatching tile
  uint32_t reference;  // CU id of the block that computed the reference's tile
  uint32_t words;      // differing 16-byte words of the tile
} gm_burnin_event_t;

// What the per-tile compare accumulates in device memory over the compares of a run, zeroed
// before the first one: 16 bytes of counters, then the log.
typedef struct gm_burnin_state {
  uint64_t total;   // differing 16-byte words
  uint32_t cursor;  // events so far; the first min(cursor, GM_BURNIN_LOG_CAP) are in log[]
  uint32_t pad;
  gm_burnin_event_t log[GM_BURNIN_LOG_CAP];  // in the order the tiles' blocks took their slots
} gm_burnin_state_t;

typedef struct gm_burnin_inject {
  uint32_t id;     // < GM_CUSCAN_IDS
  uint32_t mask;   // 1..0xFFFF
  uint32_t first;  // nonzero: the CU of the warm-up's tile 0 instead of id
} gm_burnin_inject_t;

typedef struct gm_burnin_blamed {
  uint32_t id;
  uint32_t events;        // = as_worker + as_reference
  uint32_t as_worker;     // events in which it was blamed as the worker
  uint32_t as_reference;  // ... as the reference
  uint64_t words;
} gm_burnin_blamed_t;

typedef struct gm_burnin_attr {
  uint32_t tiles, grid, step;
  uint32_t rotations;         // distinct r among the iterations
  uint32_t cus_seen;          // distinct CU ids over the warm-up's, the reference's and every
                              // iteration's map
  uint32_t tiles_moved;       // tiles some iteration computed on another CU than the reference
  uint32_t tiles_exonerated;
  uint32_t logged;            // min(events, GM_BURNIN_LOG_CAP)
  uint32_t log_overflow;      // events > logged
  uint32_t first_id;          // the CU of the warm-up's tile 0
  uint32_t inject_id;         // the id injected into; GM_CUSCAN_ANY without an injection
  uint32_t n_blamed;          // units blamed; the first min(n_blamed, blamed_cap) are stored
  uint32_t records_filled;    // min(logged, GM_BURNIN_MAX_RECORDS)
  uint64_t events;            // mismatching (iteration, tile) pairs
  gm_burnin_event_t records[GM_BURNIN_MAX_RECORDS];  // the first logged events, in log order
} gm_burnin_attr_t;

// Host only, no GPU: the blame rule over a log. Reads the first min(n_events,
// GM_BURNIN_LOG_CAP) of `events` (the rest were counted, not logged) and exonerated[0..tiles);
// stores the blamed units, most events first (ties: lower id first), and the summary fields
// events, logged, log_overflow, tiles_exonerated, n_blamed and records of *out (the others
// zero). An
// event whose tile is >= tiles or whose ids are >= GM_CUSCAN_IDS, tiles <= 0, n_events < 0,
// blamed_cap < 0 or a missing array: hipErrorInvalidValue.
int gm_probe_burn_in_blame(const gm_burnin_event_t* events, int64_t n_events,
                           const uint8_t* exonerated, int tiles, gm_burnin_attr_t* out,
                           gm_burnin_blamed_t* blamed, int blamed_cap);
// Host only: block `block` of a grid of (M / 256) · (N / 256) blocks computes tile
// (*tm, *tn) at rotation r, the map the traced kernels evaluate on the device; r = 0 is the
// plain kernels' map. *step = gm_burnin_step(grid). M, N multiples of 256, 0 <= block < grid,
// 0 <= r < grid, else hipErrorInvalidValue.
int gm_probe_burn_in_tile_map(int M, int N, int block, int r, int* tm, int* tn, int* step);
// One traced GEMM on caller-owned device buffers: gm_probe_gemm_nt's and gm_probe_mxgemm_nt's
// arguments and checks, then the rotation r, 0 <= r < grid, where each block stores its CU id
// (cu_of_tile[tile], a device pointer, 4-byte aligned, grid entries) and the injection, which
// may be NULL and whose `first` must be 0. Bad arguments: hipErrorInvalidValue before any HIP
// call. Asynchronous on `stream`.
int gm_probe_gemm_nt_traced(const void* A, const void* Bt, void* C, int M, int N, int K, int r,
                            uint32_t* cu_of_tile, const gm_burnin_inject_t* inject,
                            void* stream);
int gm_probe_mxgemm_nt_traced(int fmt, const void* A, const void* sA, const void* Bt,
                              const void* sB, void* C, int M, int N, int K, int r,
                              uint32_t* cu_of_tile, const gm_burnin_inject_t* inject,
                              void* stream);
// Registers and scratch bytes of the traced kernels: the accumulators must stay in registers
// there too, so scratch must be 0.
int gm_probe_gemm_nt_traced_info(int* num_regs, int* scratch_bytes);
int gm_probe_mxgemm_nt_traced_info(int fmt, int* num_regs, int* scratch_bytes);
// One per-tile compare on caller-owned device buffers, through the launch the burn-in's loop
// uses: a and b are n × n bf16 results (b the reference), 16-byte aligned, n a positive multiple
// of 256; cu and ref_cu the two CU maps, (n / 256)² words each; `iteration` goes into the
// events. `state` is a gm_burnin_state_t (8-byte aligned, gm_probe_burn_in_state_bytes() bytes)
// and exonerated, moved ((n / 256)² words each) and seen (GM_CUSCAN_IDS words) the three mark
// arrays, all zeroed by the caller before the first call: they accumulate over calls as over
// the iterations of a run (total and cursor grow, a mark once set stays set, events past the
// log's capacity are counted in cursor only). A missing or misaligned pointer or a bad n:
// hipErrorInvalidValue before any HIP call. Asynchronous on `stream`.
int gm_probe_count_diff_tiles(const void* a, const void* b, int n, const uint32_t* cu,
                              const uint32_t* ref_cu, uint32_t iteration, void* state,
                              uint32_t* exonerated, uint32_t* moved, uint32_t* seen,
                              void* stream);
// sizeof(gm_burnin_state_t). Host only.
uint64_t gm_probe_burn_in_state_bytes(void);
// The attributed bf16 burn-in: gm_probe_burn_in_flip's arguments, operands and meanings of
// *tflops, *mismatches and *iters, through the loop above. `inject` may be NULL. *attr and the
// first min(attr->n_blamed, blamed_cap) entries of `blamed` are filled. Bad flips, an injection
// id >= GM_CUSCAN_IDS (first == 0), a mask of 0 or above 0xFFFF, a missing attr, blamed_cap < 0
// or blamed_cap > 0 without `blamed`: hipErrorInvalidValue before any HIP call.
int gm_probe_burn_in_attr(int dev, int n, double seconds, int n_flips,
                          const uint64_t* flip_elems, const uint16_t* flip_masks,
                          const gm_burnin_inject_t* inject, double* tflops,
                          uint64_t* mismatches, int* iters, gm_burnin_attr_t* attr,
                          gm_burnin_blamed_t* blamed, int blamed_cap);
// The same for the MX burn-in (gm_probe_mx_burn_in_flip's format, operands and shapes).
int gm_probe_mx_burn_in_attr(int dev, int fmt, int n, double seconds, int n_flips,
                             const uint64_t* flip_elems, const uint16_t* flip_masks,
                             const gm_burnin_inject_t* inject, double* tflops,
                             uint64_t* mismatches, int* iters, gm_burnin_attr_t* attr,
                             gm_burnin_blamed_t* blamed, int blamed_cap);

// ------------------------------------------------------------------ lane scan
// The CU scan's frame again (one 256-thread block per CU, so one wave per SIMD; the whole LDS
// declared; the CU id read from the registers; a host-computed table compared bit for bit) around
// what neither other scan reaches: the cross-lane network, register-file addressing, the scalar
// unit, the transcendental pipe, fp64 vector arithmetic and the packed and dot instructions. Six
// tests of 4 signature words per thread t (wave w = t / 64, lane l = t % 64). The code is
// gm_lanescan_ref.h. What host and kernel share is data (hashes, operand values, menus of
// immediates, folds); the operation under test is the instruction on the device and, on the host,
// a plain model of what the ISA document says it does, so a unit that computes wrongly cannot
// produce its own expected value. H is the CU scan's hash; fold(s, v) = rotl32(s, 5) + v.
//
//   bit  name     steps per unit of iters
//     1  xlane    43 (the menu, once)
//     2  regfile   1 round
//     4  salu     16
//     8  trans     8
//    16  f64       8
//    32  packed   16
//
// xlane. x_j = H(0x300, 4 t + j), j = 0..3. Step s: j = s & 3, menu entry
// m = (s + H(0x301, 0) % 43) % 43, parameter g = H(0x301, 1 + s) (both uniform);
//   moved = move_m(old = x_{(j + 1) & 3}, src = x_j)
//   x_j   = (rotl32(moved + rotl32(x_j, 16), 9) ^ (l * 0x85EBCA6B + s)) * 0x9E3779B1
// and the signature is x_0..x_3. The menu (GM_LANESCAN_DPP_MENU, GM_LANESCAN_SWIZZLE_MENU):
//   0..28   v_mov_b32_dpp with the entry's dpp_ctrl, row_mask, bank_mask, bound_ctrl: quad_perm,
//           row_shl / row_shr / row_ror, wave_shl / rol / shr / ror :1, row_mirror,
//           row_half_mirror, row_bcast:15 (into rows 1, 3), row_bcast:31 (into rows 2, 3). A lane
//           whose row or bank (lane % 16 / 4) is masked off keeps `old`; an enabled lane whose
//           source is outside its row (or the wave) reads 0 with bound_ctrl, keeps `old` without.
//   29..33  ds_swizzle_b32: offset bit 15 set: quad perm from bits 7:0; else lane
//           ((l % 32 & and) | or) ^ xor of the lane's half, and | or << 5 | xor << 10
//   34      ds_bpermute_b32 from lane (l (g | 1) + (g >> 8)) % 64
//   35      ds_bpermute_b32 from lane ((l & g >> 14) + (g >> 20)) % 64 (many lanes read one)
//   36      ds_permute_b32 to lane (l (g | 1) + (g >> 8)) % 64: a bijection, so no two lanes
//           write one destination and no rule for collisions is relied on
//   37, 38  v_readlane_b32 of lane g % 64; v_readfirstlane_b32 (lane 0: every lane is active)
//   39      v_writelane_b32: old, with lane 21 (g % 4) set to src of lane (g >> 8) % 64
//   40, 41  v_permlane16_swap / v_permlane32_swap (vdst = old, vsrc = src): rows 1 and 3 (the upper
//           half) of vdst change places with rows 0 and 2 (the lower half) of vsrc; the result is
//           new vdst + rotl32(new vsrc, 13)
//   42      B = ballot of bit g % 32 of src: (old ^ lo(B) ^ hi(B)) + v_mbcnt (bits of B below l)
//
// regfile. A lane has 384 registers: 192 VGPRs in 6 banks of 32, indexed at run time within a
// bank, and 192 accumulation registers behind v_accvgpr_write_b32 / _read_b32. reg_r = H(0x310,
// 384 t + r). Per round q (iters rounds), with visit(r, i): s_{i & 3} = fold(s_{i & 3}, reg_r),
// reg_r = ~reg_r:
//   k = 0..11:  g = H(0x311, 16 q + k); visit(g % 192, k)                       (uniform index)
//   k = 12..15: the same g; visit(32 (g % 6) + ((g >> 8) + l) % 32, k)          (index per lane)
//   then visit(r, r) for r = 0..383 by constant index.
// After the last round s_{r & 3} = fold(s_{r & 3}, reg_r) for r = 0..383; the signature is s_0..s_3.
//
// salu. One chain per wave on uniform values; T[i] = H(0x320, i), i < 1024, is read through a
// const __restrict__ kernel argument. a = H(0x321, 4 w), b = H(0x321, 4 w + 1), c = H(0x321, 4 w +
// 2) << 32 | H(0x321, 4 w + 3); v_i = H(0x322, 4 t + i). Step s, 32-bit unless said:
//   k = T[(a ^ s) % 1024];  m = a k (64 bits);  a ^= hi(m);  b += lo(m)
//   c += b << 32 | a;  c -= k                                      (64 bits)
//   a ^= b << k % 32;  b ^= a >> (k >> 5) % 32;  a += signed(b) >> (k >> 10) % 32   (arithmetic)
//   c = rotl64(c, (k >> 15) % 32 + 1)
//   off = (k >> 20) % 16, wd = (k >> 24) % 16 + 1;  e = bits [off, off + wd) of a;  se = the
//   same bits of b, sign-extended
//   b += popcount(a) + 33 ctz(a) + 97 clz(b)                       (ctz(0) = clz(0) = 32)
//   a ^= bitreverse(b);  a = a < b ? a + e : a - se
//   b = max(b, k) - min(signed(a), signed(k));  a += |signed(a) - signed(b)|
//   a ^= lo(c);  b ^= hi(c)
//   v_{s & 3} = rotl32(v_{s & 3}, 7) + (a ^ l * 0x01000193);  v_{(s + 2) & 3} ^= b + l
// and the signature is v_0..v_3.
//
// trans. g_i = H(0x331, 4 t + i). Step s: h = H(0x330, 256 s + t), carry = g_0 & 1 (which makes
// the chain dependent); n = h % 32 - 16 + carry, neg = (h >> 5) & 1, k = (h >> 6) % 16 - 8,
// k16 = (h >> 6) % 8 - 3, m = (h >> 10) % 4096, a = (h >> 22) % 128 - 64 + carry. The bit patterns
// of these results are folded, in this order, for the operations in GM_LANESCAN_TRANS_OPS:
//   g_0: v_exp_f32(n) = 2^n;  v_log_f32(2^n) = n;  v_rcp_f32(+-2^n) = +-2^-n;
//        v_rsq_f32(4^k) = 2^-k;  v_sqrt_f32(m^2) = m
//   g_1: v_sin_f32(a / 4), v_cos_f32(a / 4) (the operand is in turns): 0, 1, 0, -1 by a % 4
//   g_2: v_rcp_f64(+-2^n), [v_sqrt_f64(4^k)], v_rsq_f64(4^k), each as lo ^ rotl32(hi, 16)
//   g_3: v_rcp_f16(2^k), v_sqrt_f16(4^k16), v_rsq_f16(4^k16)
// The host computes each by exponent arithmetic, without libm. A zero result of log, sqrt, sin and
// cos is folded as 0: its sign is not part of the test. v_sqrt_f64 is not in the chain: on an
// MI355X it returns 2^k (1 + 2^-26) at 4^k, inside its documented accuracy but not exact.
//
// f64. x = H(0x340, t) >> 6 (< 2^26), S = 0. Step s: h1 = H(0x341, 2 (256 s + t)), h2 = the next;
// a = h1 % 2^16 - 2^15, b = h2 % 2^24 - 2^23, e = (h1 >> 16) % 4, c = (h1 >> 18) % 64 + 1,
// d = h2 >> 24:
//   p = fma(x, a, b);  S += p;  r = ldexp(p, e - 3) * c + d / 8;  fl = floor(r)
//   x = fma(floor(ldexp(fl, -26)), -2^26, fl)   (= fl mod 2^26), then x = (double)(uint32_t)x
//   g_0 = fold(g_0, W(p));  g_1 = fold(g_1, W(r));
//   g_2 = fold(g_2, (x ^ (uint32_t)(8 (r - fl)) << 28) + (int32_t)ldexp(p, -12))
// and g_3 = W(S), W(v) = lo ^ rotl32(hi, 16) of v's bits. |p| < 2^42, r is below 2^52 eighths, and
// |S| <= 8 iters 2^42 < 2^53 for iters <= 255: every intermediate is an integer below 2^53 times a
// power of two, and the host computes in int64_t.
//
// packed. Step s: h_q = H(0x350, 4 (256 s + t) + q), q = 0..3.
//   v_pk_fma_f32:  acc_i += byte_i(h_0) * byte_{2 + i}(h_0), i = 0, 1 (signed bytes)
//   A_i = (h_1 >> 6 i) % 64 - 32, B_i = (h_1 >> 12 + 6 i) % 64 - 32, C_i = (h_1 >> 24 + 4 i) % 16 - 8
//   g_0 folds v_pk_fma_f16(A, B, C), then v_pk_add_f16(that, B), then v_pk_mul_f16(A, C)
//   g_1 folds, on the halves of h_2 and h_3: v_pk_mul_lo_u16, v_pk_add_u16, v_pk_sub_i16,
//       v_pk_max_i16, v_pk_min_u16
//   sdot = v_dot4_i32_i8(h_2, h_3, sdot);  udot = v_dot4_u32_u8(h_2, h_3, udot)
//   fdot = v_dot2_f32_f16(A, B, fdot);  bdot = v_dot2_f32_bf16(A, C, bdot)
// and g_2 = bits(acc_0) + rotl32(bits(acc_1), 11), g_3 = sdot ^ rotl32(udot, 8) ^ bits(fdot) ^
// rotl32(bits(bdot), 24). Every f16 value is an integer of magnitude <= 2048 and every sum is
// exact in any order: 16 iters 2^14 < 2^24 bounds iters by 63, which is GM_LANESCAN_MAX_ITERS (the
// static_asserts in gm_lanescan_ref.h hold every cap). A zero product of a negative factor is -0.
//
// Not covered: v_sqrt_f64 (above), v_cvt_scalef32_*, rounding, NaN, infinity and subnormal
// behaviour, transcendental results at points that are not exact, LDS atomics, clocks and
// thermals. The vector L1, L2, scalar and instruction caches are the cache scan's, below.
//
// The records, the injection, the per-CU entries and the result are the CU scan's, with `test`
// and `tests_failed` holding GM_LANESCAN_* bits. Arguments and the up-front hipErrorInvalidValue
// checks are those of the gm_probe_cuscan* counterparts, with 1 <= iters <= GM_LANESCAN_MAX_ITERS.
int gm_probe_lanescan_expected(uint32_t test, uint64_t seed, uint32_t iters, uint32_t* out);
// The xlane menu, menu[5 m + 0..4] = {kind, immediate, row_mask, bank_mask, bound_ctrl} of entry m
// (kind 0: DPP with the immediate as dpp_ctrl; 1: ds_swizzle with it as offset; otherwise the
// entry's own number, 34..42 as listed above), *n_menu entries (menu_cap must hold them), and the
// GM_LANESCAN_OP_* mask of the operations in the trans chain. Host only, needs no GPU.
int gm_probe_lanescan_lanes(uint32_t* menu, int menu_cap, int* n_menu, uint32_t* trans_ops);
// One block, raw. Unlike its counterparts this one returns after the block has run: the scalar
// test's table lives in a device buffer of the call's own.
int gm_probe_lanescan_signature(uint32_t test, uint64_t seed, uint32_t iters, uint32_t* dev_out,
                                uint32_t* dev_where, void* stream);
int gm_probe_lanescan(int dev, uint32_t tests_mask, uint32_t iters, uint64_t seed, int min_rounds,
                      int max_rounds, const gm_cuscan_inject_t* inject, gm_cuscan_result_t* out,
                      gm_cuscan_cu_t* cus, int cus_cap, int* n_cus);
// numRegs and localSizeBytes of the scan kernel from hipFuncGetAttributes on the current device.
// The register march is a register march only while *scratch_bytes is 0.
int gm_probe_lanescan_kernel_info(int* num_regs, int* scratch_bytes);

// ------------------------------------------------------------------ cache scan
// The CU scan's frame a fourth time, around the SRAM between the registers and HBM: the CU's
// vector L1, its XCC's L2, the scalar data cache and the instruction cache. Four tests of 4
// signature words per thread t (wave w = t / 64, lane l = t % 64); the code is
// gm_cachescan_ref.h. H is the CU scan's hash; fold(s, v) = rotl32(s, 5) + v.
//
//   bit  name    per unit of iters
//     1  l2      1 round of the march
//     2  l1      1 hit pass (the fill and the replacement sweep run once)
//     4  scalar  64 steps of the chain
//     8  icache  1 execution of the body
//
// The arena. The driver allocates blocks x GM_CACHESCAN_SEG_BYTES (64 KiB, 16384 words) of device
// memory; block b touches segment b and no other byte, so nothing depends on placement and no
// block waits for another. Word a of segment b holds P(r, a) ^ K(b), P(r, a) = H(0x400, 65536 r +
// a), K(b) = H(0x401, b). The kernel removes K(b) from what it loads before it folds: the
// signature does not depend on b, and a line served from another block's segment decodes wrongly.
// The device writes the data; the host computes the folds from scratch in an array of its own.
// A fill: thread t writes the 16-byte elements v = 256 k + t, k < 16, with plain 128-bit stores
// (plain stores keep the line in the XCC's L2); barrier.
//
// l2. Every load bypasses the vector L1 and is served by the L2: the 32-bit ones are agent-scope
// relaxed atomic loads (global_load_dword sc1), the 128-bit ones nontemporal loads
// (global_load_dwordx4 nt). s0 = s1 = s2 = s3 = 0; per round r < iters:
//   1. fill with P(r, .)
//   2. for i < 64: a = ((256 i + t) * 6151 + 3) % 16384 (a permutation: the stride is odd);
//      32-bit read g; s0 = rotl32(s0, 5) + g; s3 += (g != P(r, a)); plain write of ~g; barrier
//   3. for k < 16: 128-bit read of element v = 256 k + (t + 64) % 256, first written by the next
//      wave, and for each of its words g, c = 0..3: s1 = rotl32(s1, 7) ^ g; s2 += g;
//      s3 += (g != ~P(r, 4v + c)); barrier
// Words s0..s3; s3, the mismatches seen in flight, is 0 on a healthy unit.
//
// l1. One fill with P(64, .). A probe of word a is a plain load g1 (through the L1), then the
// 32-bit bypass load g2 of the same word: s0 = fold(s0, g1); s1 = fold(s1, g2); s2 += (g1 != g2);
// s3 += (g1 != P(64, a)). The address is made opaque to the compiler before each probe, so every
// probe is two loads.
//   (a) hit phase, iters passes over the first 16 KiB: for i < 16, j = ((64 i + l) * 389 + 11) %
//       1024, probe a = 1024 (j / 256) + 256 ((w + 1) % 4) + j % 256. Wave w filled the words with
//       (a / 256) % 4 == w, so every line is read by the wave after the one that filled it, and
//       a wave's 1024 (i, l) pairs are a permutation of its 1024 words. A pass issues its 16
//       plain loads first, then the 16 bypass loads; the folds are per probe, in the order of i.
//   (b) replacement phase, once over all 64 KiB (twice the 32 KiB the L1 is taken to hold): for
//       i < 64, a = ((256 i + t) * 4099 + 5) % 16384, probe a twice in succession.
// Words s0..s3. In the host table s0 == s1 and s2 == 0 (s3 == 0 without a poke). s0 wrong with s1
// right names the CU's L1; both wrong names the L2 or memory.
//
// scalar. T[i] = H(0x410, i), i < 8192 (32 KiB, in a buffer of its own), read through a const
// __restrict__ kernel argument at a wave-uniform index: scalar loads. Per wave i = H(0x411, 4 w) %
// 8192, a = H(0x411, 4 w + 1), b = H(0x411, 4 w + 2); v_n = H(0x412, 4 t + n). Step s < 64 iters:
//   k = T[i];  a = rotl32(a, 5) + k;  b = (b ^ a) * 0x9E3779B1;  b ^= b >> 15
//   m = ((i ^ k) + s) * 0x85EBCA6B;  m ^= m >> 13;  i = m % 8192     (the next index depends on k)
//   v_{s & 3} = rotl32(v_{s & 3}, 7) + (a ^ l * 0x01000193);  v_{(s + 2) & 3} ^= b + l
// Words v_0..v_3.
//
// icache. x = H(0x420, 2 t), y = H(0x420, 2 t + 1), sx = sy = 0. The body is
// GM_CACHESCAN_ICACHE_STEPS distinct steps in a straight line, expanded at compile time, each with
// three 32-bit literals of its own, C(j, n) = the finalizer below of 4 j + n:
//   h = (4 j + n) * 0x9E3779B1 + 0x7F4A7C15;  h ^= h >> 16;  h *= 0x85EBCA6B;  h ^= h >> 13;
//   h *= 0xC2B2AE35;  h ^= h >> 16
//   step j:  x = rotl32(x, 1 + j % 31) + C(j, 0);  x ^= y;  x *= C(j, 1) | 1
//            y = rotl32(y, 1 + (j / 31) % 31) ^ x;  y += C(j, 2)
// It is executed iters times, and after each execution sx = fold(sx, x), sy = fold(sy, y). Words
// x, y, sx, sy. The body is a function of its own that reads the program counter at its two ends:
// the difference is its span in bytes, which must be at least 128 KiB (twice the 64 KiB
// instruction cache a pair of CUs is taken to share) for the test to mean what it says.
//
// Residency is observed, never judged: thread 0 stores the shader-clock (s_memtime) counts of each
// test's first and last pass (l2: round; l1: the plain loads of a hit pass; scalar: 64 steps;
// icache: execution) to a
// side buffer [block][test][2], and the driver reports min / median / max over the blocks of the
// last round. `ok` never depends on them.
//
// Not covered: the Infinity Cache (nothing addresses it), LDS atomics, clocks and thermals; the
// L1 and instruction-cache sizes are assumptions, and a corrupted instruction may fault instead
// of computing a wrong word.
//
// The records, the injection, the per-CU entries and the result are the CU scan's, with `test`
// and `tests_failed` holding GM_CACHESCAN_* bits; 1 <= iters <= GM_CACHESCAN_MAX_ITERS. Every
// argument check comes before any HIP call.
//
// Second negative control, through the real detection path: after the named test's fill and
// barrier (l2: the first round's), thread 0 of every block XORs `mask` into word `word_offset` of
// its own segment with a plain store. For `scalar` the host flips that word of the uploaded
// table. The scan still compares with the table of a clean run, so the poked word is found by the
// test itself; gm_probe_cachescan_expected with the poke gives the exact signature of the poked
// run (a table word the chain never reads changes nothing). `icache` has no data to poke.
// hipErrorInvalidValue for a test that has no data or is not
// selected, an offset beyond the segment (16384 words) or table (8192 words), or mask == 0.
typedef struct gm_cachescan_poke {
  uint32_t test, word_offset, mask;
} gm_cachescan_poke_t;

// Shader-clock counts of the first and the last pass of test index i (bit 1 << i), as
// {min, median, max} over the blocks of the last round; 0 for a test that was not run.
typedef struct gm_cachescan_timing {
  uint64_t first[4][3];
  uint64_t last[4][3];
  uint32_t blocks;
  uint32_t pad;
} gm_cachescan_timing_t;

// The expected table of `test`, in a run with `poke` (null: none). A poke of another test leaves
// it alone. Host only, needs no GPU.
int gm_probe_cachescan_expected(uint32_t test, uint64_t seed, uint32_t iters,
                                const gm_cachescan_poke_t* poke, uint32_t* out);
// One block, raw, on an arena of its own. It returns after the block has run.
int gm_probe_cachescan_signature(uint32_t test, uint64_t seed, uint32_t iters,
                                 const gm_cachescan_poke_t* poke, uint32_t* dev_out,
                                 uint32_t* dev_where, void* stream);
// The scan. `inject`, `poke` and `timing` may be null.
int gm_probe_cachescan(int dev, uint32_t tests_mask, uint32_t iters, uint64_t seed, int min_rounds,
                       int max_rounds, const gm_cuscan_inject_t* inject,
                       const gm_cachescan_poke_t* poke, gm_cuscan_result_t* out, gm_cuscan_cu_t* cus,
                       int cus_cap, int* n_cus, gm_cachescan_timing_t* timing);
// numRegs and localSizeBytes of the scan kernel on the current device, and the span of the
// icache body in bytes, from the program counter at its two ends (one block runs the body once).
int gm_probe_cachescan_kernel_info(int* num_regs, int* scratch_bytes, int* icache_body_bytes);
// GM_CACHESCAN_SEG_BYTES, _L1_HIT_BYTES, _TABLE_BYTES, _ICACHE_STEPS. Host only.
int gm_probe_cachescan_geometry(uint32_t* seg_bytes, uint32_t* l1_hit_bytes, uint32_t* table_bytes,
                                uint32_t* icache_steps);

// ------------------------------------------------------------------ LDS scan
// The CU scan's frame a fifth time, around what sits between a lane and the cells of the CU's
// LDS (the CU scan's `lds` march proves that each cell holds a value, with 32- and 128-bit plain
// accesses only). Five tests of 4 signature words per thread t (wave w = t / 64, lane l = t %
// 64); the code is gm_ldsscan_ref.h. H is the CU scan's hash; fold(s, v) = rotl32(s, 5) + v;
// P(id, r, p, a) = H(id, (8 r + p) * 65536 + a) is word a of pass p's image in round r;
// perm(j, n, s, o) = (j s + o) % n with s odd and not a multiple of 5 (every n here is 2^k * 5),
// and j(i, q) = 256 i + (t + 64 q) % 256 is thread t's index in step i, q waves on.
//
//   bit  name    per unit of iters
//     1  width   1 round of the passes below
//     2  atomic  1 round: initial values, the three phases, the final values
//     4  bank    1 fill, 1 pass of 32-bit reads, 1 of 64-bit reads, 24 broadcast reads
//     8  tr16    1 fill and 240 transposing reads per thread
//    16  dma     1 load of all 160 KiB from the arena and its read-back
//
// width. s0..s3 = 0; per round r < iters, every pass touching each cell of the LDS once:
//   1. 8-bit stores: word a = perm(j(i,0), 40960, 12347, 7), i < 160: the four bytes of
//      P(0x500, r, 0, a), one ds_write_b8 each; barrier
//   2. halfword perm(j(i,1), 81920, 20483, 5), i < 320: zero-extended where i is even,
//      sign-extended where odd; then word perm(j(i,2), 40960, 6151, 3), i < 160; all into s0; barrier
//   3. 16-bit stores: word perm(j(i,0), 40960, 4099, 11): the two halves of P(0x500, r, 1, a); barrier
//   4. byte perm(j(i,1), 163840, 16411, 1), i < 640, zero- / sign-extended by i's parity; then the
//      8-byte cell perm(j(i,3), 20480, 8209, 9), i < 80, as one 64-bit load (low word, high
//      word); all into s1; barrier
//   5. 64-bit stores: cell perm(j(i,0), 20480, 6163, 13), words P(0x500, r, 2, .); barrier
//   6. ds_read2_b32: pair q = perm(j(i,1), 20480, 3079, 17), words x = 64 (q / 32) + q % 32 and
//      x + 32, into s2; barrier
//   7. 96-bit stores: 16-byte slot perm(j(i,0), 10240, 3083, 19), i < 40, its first three words
//      P(0x500, r, 3, .); ds_write2_b32: pair q = perm(j(i,2), 5120, 1543, 23), i < 20, the last
//      words of slots 16 (q / 8) + q % 8 and that + 8 (32 words apart); barrier
//   8. ds_read2st64_b32: pair q = perm(j(i,3), 20480, 12301, 29), words x = 128 (q / 64) + q % 64
//      and x + 64, into s2; barrier
//   9. partial overwrite: word a = perm(j(i,0), 40960, 10243, 31), v = P(0x500, r, 4, a): byte
//      v[7:0] to byte (v >> 8) & 3 of the word, then halfword v[31:16] to halfword (v >> 10) & 1;
//      barrier; word perm(j(i,1), 40960, 14341, 37) into s3; barrier
//
// atomic. A table of GM_LDSSCAN_A_TABLE_WORDS words at the start of the LDS. No signature word
// depends on the order in which lanes or waves reach a word: a returned old value is folded only
// where one thread alone touches the word, contended words are folded as final values after a
// barrier, and every contended operation commutes. Per round r: word a starts as I(r, a) =
// H(0x510, 8192 r + a) (as float(I & 1023) where f32 is added, 0 for the tickets); barrier. The
// operand of thread t, step s of slot k is O = H(0x511, ((128 r + k) * 4 + s) * 256 + t).
//   (a) private, word 256 k + t for the 13 32-bit kinds k (add, sub, inc, dec, min and max signed
//       and unsigned, and, or, xor, exchange, compare-and-swap), 8-byte word 3328 + 2 (256 k + t)
//       for the 64-bit kinds (add, signed min, unsigned max, compare-and-swap; slots 16 + 2 k and
//       + 1 for the high half), word 5376 + t for f32 add (slot 24, addend float(O & 15)): two
//       returning operations each, every old value into s0. inc and dec wrap at (O & 7) + 1; and
//       takes O | rotl32(O, 11), or takes O & rotl32(O, 11); compare-and-swap compares with the
//       initial value in step 0 (it swaps) and with ~O of step 0 in step 1 (it does not).
//   (b) contended, groups of 24 words from 5632: group 0 for all 256 threads (slots 32 + word),
//       group 1 + w for the 64 lanes of wave w (slots 64 + word). Words 0, 2, 4, 6: 64-bit add,
//       signed min, unsigned max, add by a compare-and-swap loop; 8..18: add, sub, min and max
//       signed and unsigned, and, or, xor, add by a compare-and-swap loop, f32 add. No return is
//       used. A compare-and-swap loop runs at most 256 tries; the give-ups (0: each failed try is
//       caused by one of at most 255 successes of others) are counted.
//   (c) tickets: 4 times, ticket = returning add of 1 to word 5752, then atomic or of bit
//       ticket % 32 into word 5760 + (ticket / 32) % 32. The ticket is used, never folded.
//   barrier; s1 = the thread's private words; s2 = words 0..18 of group 0, of group 1 + w, then
//   the give-ups; s3 = the counter (1024) and the 32 bitmap words (all ones); barrier.
//
// bank. The LDS as ten chunks of 4096 words. Wave-instruction g = 4 i + (w + q) % 4 of a pass
// walks chunk u = g / 64 at stride 2^k words, k = (u + r + shift) % 7: lane l of instruction m =
// g % 64 takes n = 64 m + (l + m) % 64 and word 4096 u + (n % (4096 >> k)) * 2^k + n / (4096 >>
// k). Per round: 32-bit writes of P(0x520, r, 0, a) (q = 0, shift 0; a permutation, so no two
// lanes share a word); barrier; 32-bit reads (q = 1, shift 3) into s0; 64-bit reads of 8-byte
// elements, chunks of 2048 elements, g = 4 i + (w + 2) % 4 < 320, u = g / 32, m = g % 32, k = (u
// + r) % 6 (low word into s1, high into s2); broadcasts, 8 instructions g = 4 i + w each: all
// lanes at word ((g + 32 r) * 1237 + 5) % 40960, each half h at (((g + 32 r) * 2 + h) * 3571 + 9)
// % 40960, lanes l and l + 16 at (((g + 32 r) * 32 + l % 16 + 16 (l / 32)) * 12347 + 13) % 40960,
// into s3; barrier. By the bank rule (32-bit: (a / 4) % 32, 64-bit: (a / 4) % 64, per 32-lane
// half) every conflict degree 1, 2, 4, 8, 16, 32 occurs and every lane reads from every bank.
//
// tr16. Per round: 128-bit writes of P(0x530, r, 0, .), thread t the elements 256 k + t; barrier.
// For the row strides S_k = 32, 72, 264 bytes and i < 80: the 16-lane group G = t / 16 reads
// block n = 16 i + G at origin U_k ((4099 n + 17 k + 131 r) % N_k), N_k = (163840 - 3 S_k - 32) /
// U_k + 1, U_k = 128, 8, 8 (at stride 32 the 1280 blocks tile the LDS); lane 4 q + p of the group supplies origin + q S_k + 8 p, and lane c receives elements
// (row 0..3, column c): lo = rows 0, 1, hi = rows 2, 3. s_k = fold(fold(s_k, lo), hi); s3 =
// fold(s3, lo ^ rotl32(hi, 13)); barrier.
//
// dma. The arena is 160 KiB of device memory, word a = P(0x540, 0, 0, a), shared by all blocks
// and read only. Per round wave w moves chunk c = 4 i + w (1 KiB), i < 40, to chunk d = (37 c + 11
// r + 3) % 160 of the LDS: where c + r is even with one global_load_lds_dwordx4 (lane l: the 16
// bytes of slot (l + rho) % 64, rho = (7 c + r) % 64, to d's bytes 16 l ...), where odd with four
// global_load_lds_dword (sub-chunk j: word (l + rho) % 64 of it to word l of sub-chunk (j + 1) %
// 4). s_waitcnt vmcnt(0); barrier; every word of the LDS is read back by the wave after the one
// that loaded it: s0 = fold(s0, g); s1 = rotl32(s1, 7) ^ g; s2 += g; s3 += (g != the arena's
// pattern there); barrier.
//
// Not covered: the 4-, 6- and 8-bit transposing reads, cross-lane permutes (the lane scan has
// them), any judgment of speed or of conflict cycles.
//
// The records, the injection, the per-CU entries and the result are the CU scan's, with `test`
// and `tests_failed` holding GM_LDSSCAN_* bits; 1 <= iters <= GM_LDSSCAN_MAX_ITERS. Every
// argument check comes before any HIP call.
//
// Second negative control, through the real detection path: for width, bank and tr16, after the
// test's first fill and barrier, thread 0 of every block XORs `mask` into word `word_offset` of
// the LDS, before the barrier that precedes the reads; for dma the host flips that word of the
// arena. The scan still compares with the table of a clean run; gm_probe_ldsscan_expected with
// the poke gives the exact signature of the poked run. `atomic` has no data to poke.
// hipErrorInvalidValue for atomic, a test that is not selected, an offset of 40960 or more, or
// mask == 0.
typedef struct gm_ldsscan_poke {
  uint32_t test, word_offset, mask;
} gm_ldsscan_poke_t;

// The expected table of `test`, in a run with `poke` (null: none). A poke of another test leaves
// it alone. Host only, needs no GPU.
int gm_probe_ldsscan_expected(uint32_t test, uint64_t seed, uint32_t iters,
                              const gm_ldsscan_poke_t* poke, uint32_t* out);
// One block, raw, with an arena of its own. It returns after the block has run.
int gm_probe_ldsscan_signature(uint32_t test, uint64_t seed, uint32_t iters,
                               const gm_ldsscan_poke_t* poke, uint32_t* dev_out,
                               uint32_t* dev_where, void* stream);
// The scan. `inject` and `poke` may be null.
int gm_probe_ldsscan(int dev, uint32_t tests_mask, uint32_t iters, uint64_t seed, int min_rounds,
                     int max_rounds, const gm_cuscan_inject_t* inject, const gm_ldsscan_poke_t* poke,
                     gm_cuscan_result_t* out, gm_cuscan_cu_t* cus, int cus_cap, int* n_cus);
// numRegs and localSizeBytes of the scan kernel from hipFuncGetAttributes on the current device.
int gm_probe_ldsscan_kernel_info(int* num_regs, int* scratch_bytes);
// The LDS and the arena in bytes, the atomic table in words, the three tr16 row strides in bytes.
// Host only.
int gm_probe_ldsscan_geometry(uint32_t* lds_bytes, uint32_t* arena_bytes,
                              uint32_t* atomic_table_words, uint32_t tr16_strides[3]);

// ------------------------------------------------------------------ host link (PCIe) test
// Moves checked bytes between pinned host memory and the GPU, in both directions, by the copy
// engines (hipMemcpyAsync) and by kernels that read and write host memory through its device
// mapping. Every expected value is the memtest pattern function above (same patterns, seed, pass,
// 64-bit global byte offset, inverted polarity); errors are reported in a gm_memtest_result_t.
//
// Kernel geometry (gm_hostlink.hip): `blocks` blocks (1..GM_HOSTLINK_MAX_BLOCKS) of 256 threads,
// 16-byte elements, a contiguous chunk per block rounded up to whole steps of U * 256 elements
// (U = 4 or 8 loads in flight per lane; gm_probe_hostlink_geometry reports the step in bytes), a
// 16-byte tail loop, nontemporal accesses, one wave-instruction = 1 KiB of contiguous host memory.
//
// Legs of the driver, one GM_HOSTLINK_* bit each:
//   H2D     1   hipMemcpyAsync pinned -> device        checked on the device (memtest verify)
//   D2H     2   hipMemcpyAsync device -> pinned        checked on the host
//   BIDIR   4   both at once on two streams, each to its own destination; both checks
//   KREAD   8   kernel reads pinned memory             checked in the kernel
//   KWRITE  16  kernel writes pinned memory            checked on the host
//   KDUPLEX 32  kernel copies pinned -> pinned         checked in the kernel (source) and on the
//                                                      host (destination)
// Struct layout (checked by tests/test_hostlink.py): sizeof(gm_hostlink_leg_t) = 32,
// sizeof(gm_hostlink_record_t) = 40, sizeof(gm_hostlink_result_t) = 992 with legs at byte 48,
// bidir_h2d at 240, records at 304, seconds at 944 and stage at 976.
#define GM_HOSTLINK_H2D 1
#define GM_HOSTLINK_D2H 2
#define GM_HOSTLINK_BIDIR 4
#define GM_HOSTLINK_KREAD 8
#define GM_HOSTLINK_KWRITE 16
#define GM_HOSTLINK_KDUPLEX 32
#define GM_HOSTLINK_ALL 63
#define GM_HOSTLINK_LEGS 6
#define GM_HOSTLINK_MAX_BLOCKS 1024
#define GM_HOSTLINK_MAX_RECORDS 16

typedef struct gm_hostlink_leg {
  uint64_t bytes;           // bytes the timed transfers moved (both directions where there are two)
  double ms;                // their time (device events), summed over patterns and passes
  double gbps;              // bytes / ms
  uint64_t words_in_error;
} gm_hostlink_leg_t;

typedef struct gm_hostlink_record {
  uint64_t offset;          // byte offset of the word in the buffer
  uint64_t expected;
  uint64_t got;
  uint32_t leg;             // GM_HOSTLINK_* bit
  uint32_t pattern;         // GM_MEMTEST_* bit
  uint32_t pass;
  uint32_t pad;
} gm_hostlink_record_t;

typedef struct gm_hostlink_result {
  uint64_t bytes;           // size of each of the four buffers
  uint64_t pinned_bytes;    // pinned host memory held (two buffers)
  uint64_t words_in_error;
  uint64_t bit_errors;      // sum of popcount(expected ^ got)
  uint64_t stuck_mask;      // OR of expected ^ got
  uint32_t records_filled;  // <= GM_HOSTLINK_MAX_RECORDS; later wrong words are counted only
  uint32_t legs_run;        // mask of the legs that ran to their end
  gm_hostlink_leg_t legs[GM_HOSTLINK_LEGS];  // index = log2 of the leg's bit; BIDIR: both
                                             // directions' bytes over their common window
  gm_hostlink_leg_t bidir_h2d;  // BIDIR's directions on their own (words_in_error: that side's)
  gm_hostlink_leg_t bidir_d2h;
  gm_hostlink_record_t records[GM_HOSTLINK_MAX_RECORDS];
  double seconds;           // wall time of the whole call
  double host_seconds;      // of which host fill, poison and compare
  double transfer_seconds;  // of which the transfers (warm-ups included) and the device checks
  double setup_seconds;     // of which allocating and pinning the buffers, streams and events
  char stage[16];           // what failed when the call returns an error: "args", "device",
                            // "pin", "alloc", "setup" or a leg's name; "" on success
} gm_hostlink_result_t;

// *step_bytes: bytes per block per unrolled step (U * 256 * 16); *default_blocks: the grid the
// driver uses for blocks = 0. Host only, needs no GPU. Either pointer may be NULL.
int gm_probe_hostlink_geometry(uint32_t* step_bytes, uint32_t* default_blocks);
// Tuning hook: 4 or 8 selects the kernels' loads in flight per lane (U). Returns the previous
// setting; any other value only queries.
int gm_probe_hostlink_unroll(int u);
// Kernels on caller-owned pinned host memory, on the current device. Pointers 16-byte aligned,
// `bytes` a nonzero multiple of 16, `base_offset` a multiple of 8, `pattern` one GM_MEMTEST_* bit,
// 1 <= blocks <= GM_HOSTLINK_MAX_BLOCKS, flip_offset a multiple of 8, src and dst disjoint:
// anything else is hipErrorInvalidValue before any HIP call. Then hipPointerGetAttributes must
// call the first and the last byte host memory that the device can reach, and the address the
// kernel uses is hipHostGetDevicePointer's; a device pointer or pageable memory is
// hipErrorInvalidValue (or the HIP error) and nothing is launched. One launch each, asynchronous
// on `stream` (may be NULL), except that kread and kcopy wait for their result.
// flip_mask != 0: the 64-bit word written at global byte offset flip_offset (base_offset + local
// offset) is XORed with flip_mask; what kcopy checks of its source is not affected.
int gm_probe_hostlink_kwrite(void* host_ptr, uint64_t bytes, uint32_t pattern, int invert,
                             uint64_t seed, uint32_t pass, uint64_t base_offset, int blocks,
                             uint64_t flip_offset, uint64_t flip_mask, void* stream);
// Only the error fields and bytes_tested of *out are set.
int gm_probe_hostlink_kread(const void* host_ptr, uint64_t bytes, uint32_t pattern, int invert,
                            uint64_t seed, uint32_t pass, uint64_t base_offset, int blocks,
                            void* stream, gm_memtest_result_t* out);
int gm_probe_hostlink_kcopy(const void* src_host, void* dst_host, uint64_t bytes, uint32_t pattern,
                            int invert, uint64_t seed, uint32_t pass, uint64_t base_offset,
                            int blocks, uint64_t flip_offset, uint64_t flip_mask, void* stream,
                            gm_memtest_result_t* out);
// The driver: two pinned (mapped, coherent) host buffers and two device buffers of `bytes` on
// `dev`. For each pattern of pattern_mask and each of `passes` it runs the legs of legs_mask;
// before a leg its destination holds the opposite polarity (device) or a poison fill (host), so a
// transfer that did nothing cannot pass. Only the transfers are timed (device events, `iters`
// repeats, 1..1024, after one warm-up of the same shape). blocks = 0: the default grid.
// flip_mask != 0 is the negative control: one 64-bit word of flip_leg's data (one GM_HOSTLINK_*
// bit of legs_mask) at byte offset flip_offset (multiple of 8, inside `bytes`) arrives XORed with
// flip_mask: the host source is flipped for H2D, KREAD and BIDIR (its H2D half), the device
// source for D2H (through a host round trip), and the kernel's flip argument is used for KWRITE
// and KDUPLEX. Bad arguments: hipErrorInvalidValue before any HIP call. A failed pinned
// allocation returns its HIP error with stage "pin".
int gm_probe_hostlink(int dev, uint64_t bytes, uint32_t legs_mask, uint32_t pattern_mask,
                      int passes, int iters, int blocks, uint64_t seed, uint32_t flip_leg,
                      uint64_t flip_offset, uint64_t flip_mask, gm_hostlink_result_t* out);

// ------------------------------------------------------- cross-XCC atomics and coherence test
// Checks what connects the XCCs: the memory-side atomic units behind the eight private L2s, and
// the agent-scope release/acquire hand-off between blocks of one launch (gm_atomics.hip; value
// functions and host reference: gm_atomics_ref.h, which also defines the GM_ATOMICS_* test bits,
// the GM_ATOMICS_K_* kinds and the limits). No kernel waits without a bound on another block: the
// known-answer tests do not wait at all, the CAS loop is bounded by a count a correct machine
// cannot exceed, and the hand-off's poll by wall-clock time. No result depends on where a block
// ran; XCC ids are read from HW_REG_XCC_ID and are attribution labels only.
//
// Geometry: `blocks` blocks (1..4096; 0 in the driver: multiProcessorCount) of 256 threads,
// g = 256 block + t, T = 256 blocks, T * iters <= 2^26, iters <= 1024. Every shared word is
// accessed with __hip_atomic_* at agent scope, relaxed unless stated, and is set by a
// hipMemsetAsync on the call's stream before every launch. H is the CU scan's mixer:
//   H(kind, g, s)  = H_cuscan(0x100 + kind, 1024 g + s)
//   H'(kind, g, s) = H_cuscan(0x120 + kind, 1024 g + s)        upper half of a 64-bit operand
//   a(g, s)        = (g + 97 s) mod W                          W a power of two
//
// GM_ATOMICS_ADD 1: for s < iters thread g applies one no-return operation to word a(g, s) of
// the kind's own table of W words. The operations of a kind commute, so the host fold in any
// order gives the final table exactly; a compare kernel checks it after the kernel boundary.
//   kind 0 add u32   operand H                           table starts 0
//        1 add u64   operand H' << 32 | H                0
//        2 xor u64   the same                            0
//        3 umax u32  H                                   0
//        4 umin u32  H                                   0xFFFFFFFF
//        5 and u32   ~B(H)                               0xFFFFFFFF
//        6 or  u32   B(H)                                0
//                    B(h) = 1 << (h & 31) if ((h >> 5) & 7) == 0, else 0: one bit in one
//                    operation of eight, so a word takes about a thousand operations to saturate
//        7 add f32   (float)(H % 9 - 4)                  +0.0    exact while 4 adds < 2^24
//        8 add f64   (double)(H % 9 - 4)                 +0.0    the same cap
//        9 packed bf16 add: low half H & 1, high half (H >> 1) & 1       at most 128 adds into a
//                    word: every partial sum is an integer <= 256, exact in 8 significand bits
// `spread` (a power of two, 1..65536) is the requested W. A kind with a cap uses the smallest
// power of two >= spread at which the busiest word (counted, not estimated) stays within the cap;
// for bf16 that is at least ceil(T iters / 128).
//
// GM_ATOMICS_TICKET 2: K = spread counters. For s < iters thread g draws
// old = fetch_add(ctr[k], d), k = a(g, s) with W = K, d = 1 + (H(10, g, s) & 3), and adds 1 (no
// return) to each of mark[k][old .. old + d). N_k, the host's final value of counter k, sizes
// mark[k]; the marks of all counters lie one after another. The audit kernel counts holes (a mark
// of 0), duplicates (a mark above 1) and counter_errors (ctr[k] != N_k); the draw kernel counts
// out_of_range (a ticket at or above N_k, which is not marked) and, for K <= 16, order_violations
// (a thread's tickets from one counter must strictly increase; for larger K a thread returns to a
// counter only after K draws and the order is not tracked).
//
// GM_ATOMICS_CAS 4: add u64 (operand as kind 1, with kind 11's hashes) through a compare-exchange
// loop. A thread gives up an operation, and stops, after as many failed exchanges as the host
// counted operations into that word: cas_giveups must be 0. The retries grow with the square of
// the operations into a word, so the table is widened, as for the float kinds, until no word
// takes more than 1024.
//
// GM_ATOMICS_HANDOFF 8: mailbox (b, r) is `lines` x 4 KiB of payload (lines 1 or 16; thread t
// holds words 1024 l + 4 t .. + 3 of line l) and a flag word on a 128-byte line of its own;
// E(b, r, word) = H_cuscan(0x10C, b << 20 | r << 14 | word). For r < rounds block b produces its
// mailbox (plain 16-byte stores; every wave s_waitcnt vmcnt(0); barrier; lane 0: agent release
// fence, s_waitcnt vmcnt(0), relaxed agent store of flag = own XCC id << 16 | r + 1) and then
// consumes that of p = (b + 1 + r mod (G - 1)) mod G (p = b for G = 1): every thread first
// plain-loads its payload bytes, so the lines are in its L1; lane 0 polls the flag with relaxed
// agent loads until its low half reads r + 1 or wall_clock64() has advanced budget_us; seen: lane
// 0's agent acquire fence, s_waitcnt vmcnt(0), barrier, then every thread plain-loads and
// compares every word (stale_words); not seen: unseen += 1. After the launch an audit kernel
// checks every payload word and flag again (lost_words).
//
// Negative controls (gm_atomics_inject_t, mask 0 / test 0: none):
//   ADD, CAS   (kind, a = g, b = s, mask): H of that one operation is XORed with mask
//   TICKET     (a = g, b = s): that draw marks its first slot twice
//   HANDOFF    (a = block, b = round, word, mask): that payload word is stored XORed with mask
//
// Struct layout (checked by tests/test_atomics.py): sizeof(gm_atomics_kind_t) = 40,
// sizeof(gm_atomics_record_t) = 40, sizeof(gm_atomics_inject_t) = 24,
// sizeof(gm_atomics_result_t) = 3448 with kinds at byte 32, words_in_error at 552, tickets at
// 560, cas_giveups at 608, handoffs at 616, poll_max_us at 664, pairs_observed at 680,
// pairs_stale at 1704, xcc_blocks at 2728, records_filled at 2792, records at 2800 and seconds
// at 3440.
#define GM_ATOMICS_MAX_RECORDS 16
#define GM_ATOMICS_NKINDS 13
#define GM_ATOMICS_XCC_UNKNOWN 0xFFFFFFFFu

typedef struct gm_atomics_kind {
  uint64_t ops;             // operations done
  uint64_t words_in_error;  // ADD kinds and CAS: table words that differ from the host's
  double ms;                // the kind's kernel alone (event pair)
  double gops;              // ops / ms
  uint32_t width;           // table words (ADD, CAS), counters (TICKET), mailboxes (HANDOFF)
  uint32_t pad;
} gm_atomics_kind_t;

typedef struct gm_atomics_record {
  uint64_t index;           // table word; flat mark index, then the counters; HANDOFF: mailbox << 14 | word,
                            // a flag: 1 << 40 | mailbox
  uint64_t expected;
  uint64_t got;
  uint32_t test;            // GM_ATOMICS_* bit
  uint32_t kind;            // GM_ATOMICS_K_*
  uint32_t xcc_producer;    // HANDOFF: from the flag; GM_ATOMICS_XCC_UNKNOWN elsewhere
  uint32_t xcc_consumer;    // HANDOFF, in-launch compare: the reading block's
} gm_atomics_record_t;

typedef struct gm_atomics_inject {
  uint32_t test;            // one GM_ATOMICS_* bit
  uint32_t kind;            // ADD: the kind 0..9; ignored elsewhere
  uint32_t a, b;            // g, s or block, round
  uint32_t word;            // HANDOFF: payload word < 1024 lines
  uint32_t mask;            // nonzero except for TICKET
} gm_atomics_inject_t;

typedef struct gm_atomics_result {
  uint32_t tests_run;       // mask of the tests that ran to their end
  uint32_t blocks, iters, spread, rounds, lines, budget_us;
  uint32_t xccs_seen;       // distinct XCC ids over the census launch
  gm_atomics_kind_t kinds[GM_ATOMICS_NKINDS];
  uint64_t words_in_error;  // ADD and CAS tables together
  uint64_t tickets, holes, duplicates, counter_errors, order_violations, out_of_range;
  uint64_t cas_giveups;
  uint64_t handoffs, observed, observed_cross_xcc, unseen, stale_words, lost_words;
  double poll_max_us, poll_mean_us;  // of observed hand-offs
  uint32_t pairs_observed[16][16];   // [producer XCC][consumer XCC]
  uint32_t pairs_stale[16][16];      // wrong words, booked the same way
  uint32_t xcc_blocks[16];           // blocks of the census launch per XCC
  uint32_t records_filled;  // <= GM_ATOMICS_MAX_RECORDS; later errors are counted only
  uint32_t pad;
  gm_atomics_record_t records[GM_ATOMICS_MAX_RECORDS];
  double seconds;           // wall time of the whole call
} gm_atomics_result_t;

// The host's final table of one kind: GM_ATOMICS_K_* 0..11, or 13 (GM_ATOMICS_K_COUNT) for the
// operations per word. `out` holds `width` words of 4 bytes, 8 for kinds 1, 2, 8 and 11;
// out_bytes must say exactly that. TICKET: width = K, out = N_k. Host only, needs no GPU.
// Refused (hipErrorInvalidValue): a bad geometry, a width that is no power of two or above 2^21,
// and a width at which the kind's busiest word would break its exactness cap.
int gm_probe_atomics_expected(uint32_t kind, uint32_t blocks, uint32_t iters, uint32_t width,
                              uint64_t seed, void* out, uint64_t out_bytes);
// widths[k], caps[k] (0: none) and max_adds[k] (operations into the busiest word at that width)
// per kind for a configuration; TICKET's width is `spread`, HANDOFF's entries are 0.
// Any pointer may be NULL. Host only. hipErrorInvalidValue for a bad geometry or spread, or when a
// cap cannot be kept at any width.
int gm_probe_atomics_widths(uint32_t blocks, uint32_t iters, uint32_t spread,
                            uint32_t widths[GM_ATOMICS_NKINDS], uint64_t caps[GM_ATOMICS_NKINDS],
                            uint64_t max_adds[GM_ATOMICS_NKINDS]);
// E(b, r, word) of the hand-off. Host only.
uint32_t gm_probe_atomics_payload(uint64_t seed, uint32_t block, uint32_t round, uint32_t word);
// The tests on caller-owned hipMalloc memory of the current device, on `stream` (may be NULL).
// Every buffer is set by hipMemsetAsync on the stream first. Bad arguments (geometry, alignment
// to the word size, a width that breaks a cap, an injection outside the run): hipErrorInvalidValue
// before any HIP call. add is asynchronous; the others wait for their counters and set only
// their own fields of *out (and the records).
//   add:     kind 0..9, dev_table of `width` words
//   cas:     dev_table of `width` uint64; dev_bounds `width` uint32 holding the COUNT table
//   ticket:  dev_ctr K uint32; dev_off K + 1 uint64, the prefix sums of N_k; dev_marks
//            dev_off[K] = marks uint32
//   handoff: dev_payload blocks * rounds * lines * 4096 bytes, 16-byte aligned; dev_flags
//            blocks * rounds * 128 bytes
int gm_probe_atomics_add(uint32_t kind, void* dev_table, uint32_t width, uint32_t blocks,
                         uint32_t iters, uint64_t seed, const gm_atomics_inject_t* inject,
                         void* stream);
int gm_probe_atomics_cas(void* dev_table, const void* dev_bounds, uint32_t width, uint32_t blocks,
                         uint32_t iters, uint64_t seed, const gm_atomics_inject_t* inject,
                         void* stream, gm_atomics_result_t* out);
int gm_probe_atomics_ticket(void* dev_ctr, const void* dev_off, void* dev_marks, uint64_t marks,
                            uint32_t counters, uint32_t blocks, uint32_t iters, uint64_t seed,
                            const gm_atomics_inject_t* inject, void* stream,
                            gm_atomics_result_t* out);
int gm_probe_atomics_handoff(void* dev_payload, void* dev_flags, uint32_t blocks, uint32_t rounds,
                             uint32_t lines, uint32_t budget_us, uint64_t seed,
                             const gm_atomics_inject_t* inject, void* stream,
                             gm_atomics_result_t* out);
// The driver: the tests of tests_mask on device `dev` with its own buffers, on the default
// stream. blocks = 0: multiProcessorCount. `inject` (may be NULL) must name a test of tests_mask
// and a place inside the run. Bad arguments: hipErrorInvalidValue before any HIP call (with
// blocks = 0, what depends on the block count is checked once the device has been asked).
int gm_probe_atomics(int dev, uint32_t tests_mask, uint32_t blocks, uint32_t iters,
                     uint32_t spread, uint32_t rounds, uint32_t lines, uint32_t budget_us,
                     uint64_t seed, const gm_atomics_inject_t* inject, gm_atomics_result_t* out);

// ------------------------------------------------------- host-GPU atomics and hand-off test
// Checks how a tenant's host code and its kernels synchronise: system-scope atomics on pinned
// host memory, which travel as PCIe AtomicOps, and release/acquire hand-offs through flags in
// host memory, in both directions, while a kernel runs (gm_hostsync.hip; value functions and
// audits: gm_hostsync_ref.h, which defines the GM_HOSTSYNC_* test bits and limits; the host
// threads' side, plain C++: gm_hostsync_host.h). It is per link, not per CU.
//
// Memory: every shared word (tables, counters, marks, flags, mailboxes) lies in
// hipHostMalloc(Mapped | Coherent) memory, zeroed by the host before the launch, and the kernels
// reach it through hipHostGetDevicePointer. The GPU side uses __hip_atomic_* at
// __HIP_MEMORY_SCOPE_SYSTEM, the host side the __atomic_* builtins on the same words, relaxed
// unless stated. Only what PCIe carries natively is exercised: fetch-add (32 and 64 bit, with
// and without return), swap and compare-and-swap. hipDeviceAttributeHostNativeAtomicSupported is
// reported as atomics_supported; where it is 0 the four atomic tests are not launched and are
// listed in tests_skipped.
//
// Participants: `blocks` GPU blocks of 256 threads (1 .. CU count; 0 in the driver:
// min(16, CUs)) and `host_threads` std::threads (0..8) inside the entry point, joined on every
// return path, which make no HIP call. In the atomic tests host thread j plays block blocks + j:
// it walks t < 256, s < iters with the same value functions, concurrently with the kernel. So
// with B = blocks + host_threads the expected tables are those of the atomics test over B blocks
// (H, a(g, s), op64, the draw, the CAS width rule: gm_atomics_ref.h), g = 256 block + t.
// B * 256 * iters <= 2^20, iters <= 1024. A host thread starts when it reads the `ready` word the
// kernel stores (system scope) at its start, or after 2 s. host_ops_in_flight counts the host
// operations made while the kernel's end event was still hipErrorNotReady; it is informational.
//
// GM_HOSTSYNC_ADD 1: no-return fetch-add, u32 and u64 (atomics kinds 0 and 1), each into a table
// of `spread` words; the final table equals the host fold, compared on the host after the join.
// GM_HOSTSYNC_TICKET 2: as GM_ATOMICS_TICKET with K = spread counters and the marks in host
// memory, GPU and host drawing from the same counters; the host audits holes, duplicates and
// counter_errors; out_of_range is counted by whoever drew the ticket.
// GM_HOSTSYNC_SWAP 4: operation (g, s) does old = exchange(word[a(g, s)], token),
// token = 1 + 1024 g + s (u32), W = spread, and records old (a device buffer for GPU threads, a
// host vector for played ones). Per word w the returned values of the operations into w plus the
// final word[w] must be the tokens of those operations plus one 0, each once: swap_missing (a
// token or the 0 is absent), swap_duplicates (a value seen n > 1 times: n - 1), swap_foreign (a
// value that is no token of that word).
// GM_HOSTSYNC_CAS 8: as GM_ATOMICS_CAS over B blocks, the table widened by the same rule; a
// participant gives an operation up after as many failed exchanges as the host counted
// operations into that word (every failure implies another's success, whoever contends).
// GM_HOSTSYNC_HANDOFF 16: a ping-pong per block; host thread b mod host_threads serves block b
// (host_threads >= 1). Every round has its own flag words, each on a 128-byte line of its own,
// none reused; a payload is `lines` x 4 KiB (1 or 16),
//   E(dir, b, r, word) = H_cuscan(0x600 + dir, b << 20 | r << 14 | word)    dir 0: host to device
// For r < rounds: (1) the host plain-stores E(0, b, r, .) and store-releases flagH[b][r] = r + 1;
// (2) the block: every thread plain-loads its payload bytes; lane 0 polls flagH[b][r] with
// relaxed system loads until it reads r + 1 or wall_clock64() has advanced budget_us; seen: lane
// 0's system acquire fence, s_waitcnt vmcnt(0), barrier, every thread plain-loads and compares
// every word (stale_words of direction 0); not seen: unseen += 1, the block goes on; (3) the
// block plain-stores E(1, b, r, .) to its host mailbox, 16 bytes per thread per line; every wave
// s_waitcnt vmcnt(0); barrier; lane 0: system release fence, s_waitcnt vmcnt(0), relaxed system
// store of flagD[b][r] = seen << 16 | r + 1; (4) the host polls flagD[b][r] with acquire loads
// until its low half reads r + 1 or host_budget_us of steady_clock have passed; seen: it compares
// every word (stale_words of direction 1); not seen: unseen += 1 and on to r + 1. After the join
// and the stream's end the host audits every payload word and flag of both directions again
// (lost_words). An unseen hand-off is legal. poll_max_us is the longest poll that ended in a
// flag seen (taken before the last load); rtt_* the host-measured time from the flag store of
// (1) to the flag seen in (4). Worst case for the kernel: rounds * budget_us, rounds <= 64,
// budget_us <= 20000.
//
// Negative controls (gm_hostsync_inject_t; NULL: none). For ADD, TICKET, SWAP and CAS a = g may
// name a host-played thread (g >= 256 blocks), which exercises the host path.
//   ADD, CAS   (kind, a = g, b = s, mask): H of that one operation is XORed with mask
//   TICKET     (a = g, b = s): that draw marks its first slot twice
//   SWAP       (a = g, b = s, mask): that operation stores its token XOR mask
//   HANDOFF    (kind = direction, a = block, b = round, word, mask): the producer stores that
//              payload word XORed with mask
//
// Struct layout (checked by tests/test_hostsync.py): sizeof(gm_hostsync_record_t) = 40,
// sizeof(gm_hostsync_inject_t) = 24, sizeof(gm_hostsync_dir_t) = 40,
// sizeof(gm_hostsync_result_t) = 968 with words_in_error at byte 48, tickets at 80, swaps at 120,
// cas_giveups at 152, host_ops_in_flight at 160, lost_words at 168, dir at 176, rtt_median_us at
// 256, ms at 272, records_filled at 312, records at 320 and seconds at 960.
#define GM_HOSTSYNC_MAX_RECORDS 16
#define GM_HOSTSYNC_WHERE_STALE 1u   /* HANDOFF: found by the consumer while the kernel ran */
#define GM_HOSTSYNC_WHERE_LOST 2u    /* HANDOFF: found by the audit after the launch */

typedef struct gm_hostsync_record {
  uint64_t index;           // table word; flat mark index, then the counters; SWAP: the word;
                            // HANDOFF: block << 20 | round << 14 | word, a flag:
                            // 1 << 40 | block << 6 | round
  uint64_t expected;
  uint64_t got;             // SWAP: the value that is foreign, missing or doubled there
  uint32_t test;            // GM_HOSTSYNC_* bit
  uint32_t kind;            // ADD: 0 u32, 1 u64; HANDOFF: the direction; 0 elsewhere
  uint32_t where;           // HANDOFF: GM_HOSTSYNC_WHERE_*; 0 elsewhere
  uint32_t pad;
} gm_hostsync_record_t;

typedef struct gm_hostsync_inject {
  uint32_t test;            // one GM_HOSTSYNC_* bit
  uint32_t kind;            // ADD: the kind 0..1; HANDOFF: the direction 0..1; ignored elsewhere
  uint32_t a, b;            // g, s or block, round
  uint32_t word;            // HANDOFF: payload word < 1024 lines
  uint32_t mask;            // nonzero except for TICKET
} gm_hostsync_inject_t;

typedef struct gm_hostsync_dir {
  uint64_t handoffs, observed, unseen, stale_words;
  double poll_max_us;       // of observed hand-offs
} gm_hostsync_dir_t;

typedef struct gm_hostsync_result {
  uint32_t tests_run;       // mask of the tests that ran to their end
  uint32_t tests_skipped;   // asked for and not launched: atomics_supported is 0
  uint32_t atomics_supported;
  uint32_t blocks, host_threads, iters, spread, rounds, lines, budget_us, host_budget_us;
  uint32_t cas_width;       // the CAS table's words
  uint64_t words_in_error;  // ADD and CAS tables together
  uint64_t add_u32_errors, add_u64_errors, cas_errors;
  uint64_t tickets, holes, duplicates, counter_errors, out_of_range;
  uint64_t swaps, swap_missing, swap_duplicates, swap_foreign;
  uint64_t cas_giveups;
  uint64_t host_ops_in_flight;
  uint64_t lost_words;
  gm_hostsync_dir_t dir[2];  // 0: host to device (seen by the kernel), 1: device to host
  double rtt_median_us, rtt_max_us;
  double ms[5];             // wall time of each test's launches: ADD, TICKET, SWAP, CAS, HANDOFF
  uint32_t records_filled;  // <= GM_HOSTSYNC_MAX_RECORDS; later errors are counted only
  uint32_t pad;
  gm_hostsync_record_t records[GM_HOSTSYNC_MAX_RECORDS];
  double seconds;           // wall time of the whole call
} gm_hostsync_result_t;

// The host's expectation for B = blocks + host_threads blocks. kind 0, 1 (ADD), 10 (TICKET: N_k),
// 11 (CAS) and 13 (operations per word): the atomics test's table of `width` words (8 bytes for
// kinds 1 and 11, else 4). kind 14 (swap): B * 256 * iters uint64, word << 32 | token of
// operation g * iters + s. out_bytes must say exactly that. Host only, needs no GPU.
int gm_probe_hostsync_expected(uint32_t kind, uint32_t blocks, uint32_t host_threads,
                               uint32_t iters, uint32_t width, uint64_t seed, void* out,
                               uint64_t out_bytes);
// The CAS table's width for a requested spread. Host only.
int gm_probe_hostsync_cas_width(uint32_t blocks, uint32_t host_threads, uint32_t iters,
                                uint32_t spread, uint32_t* width);
// E(dir, b, r, word) of the hand-off. Host only.
uint32_t gm_probe_hostsync_payload(uint64_t seed, uint32_t dir, uint32_t block, uint32_t round,
                                   uint32_t word);
// hipDeviceAttributeHostNativeAtomicSupported of device `dev`.
int gm_probe_hostsync_supported(int dev, int* supported);
// One test on the current device with its own pinned memory, on `stream` (may be NULL); each
// waits for its launch and its host threads and sets its own fields of *out. Bad arguments
// (geometry, a width that breaks the CAS cap, an injection outside the run): hipErrorInvalidValue
// before any HIP call; blocks above the CU count: the same, once the device has been asked.
// table_out (may be NULL) takes the final table: `width` words of 4 bytes, 8 for kind 1 and cas.
int gm_probe_hostsync_add(uint32_t kind, uint32_t blocks, uint32_t host_threads, uint32_t iters,
                          uint32_t width, uint64_t seed, const gm_hostsync_inject_t* inject,
                          void* stream, void* table_out, gm_hostsync_result_t* out);
int gm_probe_hostsync_ticket(uint32_t blocks, uint32_t host_threads, uint32_t iters,
                             uint32_t counters, uint64_t seed, const gm_hostsync_inject_t* inject,
                             void* stream, gm_hostsync_result_t* out);
int gm_probe_hostsync_swap(uint32_t blocks, uint32_t host_threads, uint32_t iters, uint32_t width,
                           uint64_t seed, const gm_hostsync_inject_t* inject, void* stream,
                           gm_hostsync_result_t* out);
int gm_probe_hostsync_cas(uint32_t blocks, uint32_t host_threads, uint32_t iters, uint32_t width,
                          uint64_t seed, const gm_hostsync_inject_t* inject, void* stream,
                          void* table_out, gm_hostsync_result_t* out);
int gm_probe_hostsync_handoff(uint32_t blocks, uint32_t host_threads, uint32_t rounds,
                              uint32_t lines, uint32_t budget_us, uint32_t host_budget_us,
                              uint64_t seed, const gm_hostsync_inject_t* inject, void* stream,
                              gm_hostsync_result_t* out);
// The driver: the tests of tests_mask on device `dev` with its own buffers and stream. blocks = 0:
// min(16, multiProcessorCount). `inject` (may be NULL) must name a test of tests_mask that is run
// and a place inside the run. The hand-off needs host_threads >= 1. Bad arguments:
// hipErrorInvalidValue before any HIP call (what depends on the CU count is checked once the
// device has been asked).
int gm_probe_hostsync(int dev, uint32_t tests_mask, uint32_t blocks, uint32_t host_threads,
                      uint32_t iters, uint32_t spread, uint32_t rounds, uint32_t lines,
                      uint32_t budget_us, uint32_t host_budget_us, uint64_t seed,
                      const gm_hostsync_inject_t* inject, gm_hostsync_result_t* out);

#ifdef __cplusplus
}
static_assert(sizeof(gm_hostsync_record_t) == 40 && sizeof(gm_hostsync_inject_t) == 24 &&
                  sizeof(gm_hostsync_dir_t) == 40 && sizeof(gm_hostsync_result_t) == 968,
              "gm_hostsync_* layout");
static_assert(__builtin_offsetof(gm_hostsync_result_t, words_in_error) == 48 &&
                  __builtin_offsetof(gm_hostsync_result_t, tickets) == 80 &&
                  __builtin_offsetof(gm_hostsync_result_t, swaps) == 120 &&
                  __builtin_offsetof(gm_hostsync_result_t, cas_giveups) == 152 &&
                  __builtin_offsetof(gm_hostsync_result_t, dir) == 176 &&
                  __builtin_offsetof(gm_hostsync_result_t, rtt_median_us) == 256 &&
                  __builtin_offsetof(gm_hostsync_result_t, ms) == 272 &&
                  __builtin_offsetof(gm_hostsync_result_t, records) == 320 &&
                  __builtin_offsetof(gm_hostsync_result_t, seconds) == 960,
              "gm_hostsync_result_t layout");
static_assert(sizeof(gm_atomics_kind_t) == 40 && sizeof(gm_atomics_record_t) == 40 &&
                  sizeof(gm_atomics_inject_t) == 24 && sizeof(gm_atomics_result_t) == 3448,
              "gm_atomics_* layout");
static_assert(__builtin_offsetof(gm_atomics_result_t, kinds) == 32 &&
                  __builtin_offsetof(gm_atomics_result_t, tickets) == 560 &&
                  __builtin_offsetof(gm_atomics_result_t, handoffs) == 616 &&
                  __builtin_offsetof(gm_atomics_result_t, pairs_observed) == 680 &&
                  __builtin_offsetof(gm_atomics_result_t, records) == 2800 &&
                  __builtin_offsetof(gm_atomics_result_t, seconds) == 3440,
              "gm_atomics_result_t layout");
#endif
