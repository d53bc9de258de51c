/*
 * vmnhip.h — C ABI of the MI355X-native exponentiation / re-encryption / proof-of-shuffle core
 * for the Verificatum Mix-Net.
 *
 * This is the drop-in boundary.  The reference (verificatum-vmn, Java) reaches its
 * arithmetic through the array classes of VCR 3.1.0 (com.verificatum.arithm.PGroupElementArray,
 * PRingElementArray, LargeIntegerArray, ...), which are not part of the reference tree; the reference's
 * own files only show the *call sites*.  Every entry point below is one such array-level call, and
 * its comment cites the reference call site(s) it serves ("ref:" = path under /root/reference,
 * P/ = src/java/com/verificatum/protocol/).  A JNI shim maps `long` handles and `byte[]` onto these
 * functions one-to-one.
 *
 * Conventions
 *   - Plain C, no C++/torch types.  Handles are opaque pointers.
 *   - Every function returns VMN_OK (0) or a negative vmn_status; nothing throws or aborts
 *     (the reference replaces malformed inputs by trivial values and carries on:
 *     ref: P/hvzk/PoSBasicTW.java:794-815, P/mixnet/ShufflerElGamalSession.java:207-214).
 *   - Verdicts and membership results are returned through int* out-parameters (1 / 0).
 *   - Host byte buffers use the reference's wire format for fixed-width integers: big-endian,
 *     `nbytes` bytes per value, values concatenated (the payload of the byte-tree leaves,
 *     SURVEY.md App. D).  Arrays live on the device; results are fresh arrays (the reference's
 *     arrays are immutable, ref: P/hvzk/PoSBasicTW.java:1088-1101 for the explicit free()s).
 *   - All work is enqueued on the context's HIP stream; functions that return host data
 *     synchronise that stream.  Calls on distinct contexts are independent; calls on one context
 *     must be serialised by the caller (one protocol thread per party, SURVEY.md §8b "Threading").
 *   - There is NO CPU fallback: if no gfx950 device is usable, vmn_ctx_create fails with
 *     VMN_ERR_DEVICE and nothing else can be called.
 */
#ifndef VMNHIP_H
#define VMNHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum vmn_status {
    VMN_OK = 0,
    VMN_ERR_ARG = -1,       /* null/invalid handle, size mismatch, unsupported modulus size */
    VMN_ERR_DEVICE = -2,    /* HIP error (no device, launch failure); see vmn_last_error() */
    VMN_ERR_NOMEM = -3,     /* device or host allocation failed */
    VMN_ERR_FORMAT = -4,    /* value out of range on import (>= modulus) */
    VMN_ERR_UNSUPPORTED = -5
} vmn_status;

typedef struct vmn_ctx vmn_ctx;         /* one GPU + one stream + scratch workspace            */
typedef struct vmn_group vmn_group;     /* ModPGroup: subgroup of order q of Z_p^*, generator g */
typedef struct vmn_garray vmn_garray;   /* PGroupElementArray over a vmn_group (device)         */
typedef struct vmn_rarray vmn_rarray;   /* PRingElementArray / PFieldElementArray over Z_q       */

/* ---- library / context ------------------------------------------------------------------- */

const char* vmn_version(void);
/* Thread-local description of the last failing call in this thread (never NULL). */
const char* vmn_last_error(void);
/* for libraries layered on this ABI (vmnproofs.h): record the message vmn_last_error() returns */
void vmn_report_error(const char* message);

/* device: HIP device ordinal.  Fails with VMN_ERR_DEVICE when no gfx950 GPU is present. */
int vmn_ctx_create(int device, vmn_ctx** out);
void vmn_ctx_destroy(vmn_ctx* ctx);
/* Use an externally owned hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL = the
 * context's own stream. */
int vmn_ctx_set_stream(vmn_ctx* ctx, void* hip_stream);
void* vmn_ctx_get_stream(vmn_ctx* ctx);
int vmn_ctx_synchronize(vmn_ctx* ctx);
/* The helper thread.  The reference runs ONE helper thread beside a party's protocol thread: it multiplies and permutes
 * the next input while the protocol thread verifies a proof (ref: P/mixnet/ShufflerElGamalSession.java:839-859, 894-944),
 * or writes byte trees (P/hvzk/CCPoSW.java:114-123).  A thread that calls vmn_ctx_helper_begin(ctx) becomes that helper
 * until vmn_ctx_helper_end(ctx): its calls on arrays / groups of ctx run on a second, high-priority stream with its own
 * pool, scratch and lock, so they neither wait for the protocol thread's calls nor queue behind its kernels (the long
 * fixed-base launches are one workgroup per tile so that slots free up every few milliseconds).
 * Ordering.  vmn_ctx_helper_mark (either thread) records "everything the protocol thread has queued up to here"; begin()
 * and helper_sync() order the helper's stream behind the LATEST mark (begin() sets one if there has never been any) --
 * not behind work queued after it, which is what lets the helper run beside that work.  The protocol thread marks right
 * after queueing what the helper needs (typically just before it starts the thread); end() waits for the helper's work,
 * so the protocol thread may use its results after joining the thread.  An array must not be freed by one thread while
 * the other still uses it -- the reference's rule for its own arrays.  One helper per context. */
int vmn_ctx_helper_mark(vmn_ctx* ctx);
int vmn_ctx_helper_begin(vmn_ctx* ctx);
int vmn_ctx_helper_sync(vmn_ctx* ctx);
int vmn_ctx_helper_end(vmn_ctx* ctx);
/* Number of compute units of the context's device (used by the benchmark to state the roofline). */
int vmn_ctx_num_cus(vmn_ctx* ctx);
/* Small arrays.  One element per lane fills the device only from ~1.3 x 10^5 elements on; real elections (the
 * reference's demo: 10^4 ciphertexts, BASELINE.json configs[0]) are far below.  For 2048-bit moduli every launch over at
 * most `items` elements therefore runs in the WIDE geometry -- the same rows, same results, four lanes per element, so
 * that each chain of dependent products is ~2.5 times shorter.  Default 40960 (the measured crossover; env
 * VMN_WIDE_MAX overrides it); 0 = never, SIZE_MAX = always.  A tuning knob: results never depend on it. */
int vmn_ctx_set_small_array_threshold(vmn_ctx* ctx, size_t items);
/* The same one step further: launches over at most `items` elements of a 2048-bit modulus spread every element over
 * EIGHT lanes (default 6144 elements, env VMN_WIDE8_MAX; 0 = never).  Takes precedence over the threshold above. */
int vmn_ctx_set_tiny_array_threshold(vmn_ctx* ctx, size_t items);
/* Memory accounting (operations / leak hunting): bytes and blocks of freed arrays cached for reuse, bytes of live
 * allocations handed out and not yet freed (arrays + temporaries), and a group's cached fixed-base tables. */
int vmn_ctx_memory_stats(vmn_ctx* ctx, size_t* pool_bytes, size_t* pool_blocks, size_t* live_bytes);
size_t vmn_group_table_bytes(const vmn_group* grp);

/* ---- groups -------------------------------------------------------------------------------
 * ModPGroup(p, q, g): ref: P/elgamal/ProtocolElGamal.java:738-800 (group shapes), the marshalled
 * example at demo/mixnet/benchmarks/bench_config:43.  p, q, g are big-endian, nbytes each.
 * Supported modulus sizes: 512, 1024, 2048, 3072, 4096 bits, and -- for completeness, untuned (the reference offers safe
 * primes up to 15 424 bits and benchmarks with a 15 492-bit group) -- 8192 and 16384 bits (a modulus runs in the smallest
 * size that holds it). */
int vmn_modp_group_create(vmn_ctx* ctx, const uint8_t* p_be, const uint8_t* q_be, const uint8_t* g_be,
                          size_t nbytes, vmn_group** out);
/* ECqPGroup over a named prime curve, any of the 26 names the reference offers (demo/mixnet/.conf:151-176; 19 distinct
 * curves, all of cofactor 1): "P-256" and "P-384" -- the two north_star names, with the field primes compiled into the
 * kernels (csrc/ec_kernels.h FieldPrime) -- "P-224" (the curve the reference runs its own `check` on,
 * demo/mixnet/.checkbaseconf:59; square roots by Tonelli-Shanks, p = 1 mod 4), "P-521" (benchmarks/bench_config:37), "P-192";
 * the aliases "secp192r1", "prime192v1", "secp224r1", "secp256r1", "prime256v1", "secp384r1", "secp521r1" of these; and, on
 * the kernels for a general a (dbl-2007-bl, the prime taken at run time), "brainpoolp192r1", "brainpoolp224r1",
 * "brainpoolp256r1", "brainpoolp320r1", "brainpoolp384r1", "brainpoolp512r1" (OpenSSL's "brainpoolP256r1" spelling is
 * accepted too), "prime192v2", "prime192v3", "prime239v1", "prime239v2", "prime239v3", "secp192k1", "secp224k1" and
 * "secp256k1".  Only P-256 and P-384 are tuned.  Any other name is VMN_ERR_UNSUPPORTED.
 * ref: the default group of the reference, demo/mixnet/.conf:153 (P-256); SURVEY.md §2.3 K11.  Group elements cross the boundary as
 * x || y (elem_bytes = 2 * coordinate width, big-endian; the point at infinity is all 0xff bytes);
 * exponents are residues mod the group order, exp_bytes wide (the width of the order: secp224k1 has 225 bits of order
 * on a 224-bit field).  Every vmn_garray_* call works on such groups with the
 * group operation = point addition ("mul") and exponentiation = scalar multiplication ("exp"). */
int vmn_ec_group_create(vmn_ctx* ctx, const char* curve_name, vmn_group** out);
void vmn_group_destroy(vmn_group* grp);
size_t vmn_group_elem_bytes(const vmn_group* grp);     /* bytes per group element on the wire */
size_t vmn_group_exp_bytes(const vmn_group* grp);      /* bytes per exponent (ring element) on the wire */
/* The two widths are those the group was created with until this is called (vmn_modp_group_create: nbytes for both;
 * curves: the coordinate size).  0 selects the reference's own width, the length of Java's
 * BigInteger.toByteArray() of the modulus resp. the order -- floor(bits / 8) + 1, e.g. 257-byte elements and 256-byte
 * exponents for an RFC 3526 2048-bit group, 33 / 33 for P-256 -- which is what VCR writes into byte-tree leaves
 * (the 15 492-bit group of demo/mixnet/benchmarks/bench_config:43 has 1 937-byte leaves).  A JNI
 * binding calls this with (0, 0) right after creating the group.  Must precede any other use of the group. */
int vmn_group_set_wire_bytes(vmn_group* grp, size_t elem_bytes, size_t exp_bytes);
/* PGroup accessors used by host-side protocol code: getElementOrder() (P/hvzk/PoSBasicTW.java:470 uses its
 * bit length), getg() (P/mixnet/PermutationCommitment.java:200), and the modulus / field prime.
 * kind: 0 = ModPGroup, 1 = ECqPGroup.  order: exp_bytes big-endian bytes; modulus: the modulus resp. the field prime (the
 * width of one element resp. one coordinate); generator: elem_bytes.  curve_a (ECqPGroup only): the coefficient a of
 * y^2 = x^3 + a x + b as a residue in [0, p), one coordinate's width (p - 3 for the NIST curves). */
int vmn_group_kind(const vmn_group* grp);
vmn_ctx* vmn_group_ctx(const vmn_group* grp);        /* the context (main lane) the group was created in */
int vmn_group_get_order(const vmn_group* grp, uint8_t* q_be);
int vmn_group_get_modulus(const vmn_group* grp, uint8_t* p_be);
int vmn_group_get_generator(const vmn_group* grp, uint8_t* g_be);
int vmn_group_get_curve_a(const vmn_group* grp, uint8_t* a_be);

/* ---- group element arrays (PGroupElementArray) --------------------------------------------- */

/* pGroup.toElementArray(size, reader) / unsafeToElementArray: import n fixed-width big-endian
 * values.  ref: P/hvzk/PoSBasicTW.java:507, 787-792; P/mixnet/ShufflerElGamalSession.java:205.
 * *all_in_range (may be NULL) is set to 0 if some value is >= p or == 0 (the array is then
 * still created, offending entries replaced by 1, mirroring the reference's "replace by trivial
 * value" convention); subgroup membership proper is vmn_garray_is_member. */
int vmn_garray_from_be(vmn_group* grp, const uint8_t* be, size_t n, vmn_garray** out, int* all_in_range);
/* array.toByteTree() payload: n * elem_bytes big-endian bytes.  ref: 174 toByteTree call sites, e.g.
 * P/hvzk/PoSBasicTW.java:694-699. */
int vmn_garray_to_be(const vmn_garray* a, uint8_t* be_out);
/* The same in the reference's byte-tree framing: node(N leaves of elem_bytes) =
 * 00 | uint32_be(N) | N x (01 | uint32_be(elem_bytes) | value); over a curve group N x node(leaf(x), leaf(y)), the point at
 * infinity as two leaves of 0xff bytes (= -1) [NOT-IN-REF: VCR's form, from the verifier specification].  Headers are written / checked on the
 * GPU.  from_bytetree: expected_n = 0 accepts any size (pGroup.toElementArray(0, reader)); *format_ok = 0
 * (and no array) when the tree is not a node of leaves of the right width (the reference's
 * ArithmFormatException / EIOException, which its callers catch: P/hvzk/PoSBasicTW.java:505-513). */
size_t vmn_garray_bytetree_size(const vmn_garray* a);
int vmn_garray_to_bytetree(const vmn_garray* a, uint8_t* out);
int vmn_garray_from_bytetree(vmn_group* grp, const uint8_t* bt, size_t len, size_t expected_n, vmn_garray** out,
                             int* format_ok, int* all_in_range);
size_t vmn_rarray_bytetree_size(const vmn_rarray* a);
int vmn_rarray_to_bytetree(const vmn_rarray* a, uint8_t* out);
int vmn_rarray_from_bytetree(vmn_group* grp, const uint8_t* bt, size_t len, size_t expected_n, vmn_rarray** out,
                             int* format_ok, int* all_in_range);
/* Ciphertext lists in the reference's `native` interface (its default: ProtocolElGamalInterfaceNative / ...SeqHex,
 * CiphertextReaderLine / CiphertextWriterLine; `vmnc -ciphs -ini native -outi raw` is the first command of an election): one
 * ciphertext per line, the line being the hexadecimal byte tree of that ciphertext alone -- node(u, v) with u, v element trees
 * at width 1 and node(width element trees) above; an element tree is leaf(elem_bytes) resp. node(leaf(x), leaf(y)).  B bytes
 * = 2 B digits per line, B = vmn_hexlines_line_bytes (0 for a null group or a width of 0 or above 65536): 527 for a 2048-bit
 * group at 256-byte leaves and width 1, 501 for P-256 at 33-byte coordinates and width 3.  The widths are the group's wire widths.
 * Lines end as Java's readLine ends them (\n, \r, or \r\n counted once; text behind the last terminator is a line if it is
 * not empty); they are found, decoded and checked on the GPU and converted by the import kernels of the byte trees.
 * from_hexlines: out receives the 2 * width component arrays u_1..u_width, v_1..v_width of *n_out elements each.  *format_ok = 0,
 * every out[] slot NULL and *first_bad_line = the zero-based index of the first defective line when a line has not exactly 2 B
 * digits 0-9a-fA-F or its framing is not this group's and width's; a line count that differs from a non-zero expected_n is the
 * same with *first_bad_line = min(lines, expected_n).  [NOT-IN-REF: the reference rejects the whole file as well, without naming
 * the line; it is silent on the case of the digits (either is read, lowercase written), and fails on a blank line, as here.]
 * Values >= p, zero, or off the curve: as vmn_garray_from_bytetree (arrays created, entries replaced, *all_in_range = 0,
 * may be NULL); subgroup membership is vmn_garray_is_member.  A text without lines gives 2 * width empty arrays.
 * to_hexlines writes vmn_garrays_hexlines_size = n (2 B + 1) bytes: lowercase digits, every line ended by \n, no NUL. */
size_t vmn_hexlines_line_bytes(const vmn_group* grp, size_t width);
int vmn_garrays_from_hexlines(vmn_group* grp, size_t width, const char* text, size_t len, size_t expected_n, vmn_garray** out,
                              size_t* n_out, int* format_ok, size_t* first_bad_line, int* all_in_range);
size_t vmn_garrays_hexlines_size(const vmn_garray* const* comps, size_t width);
int vmn_garrays_to_hexlines(const vmn_garray* const* comps, size_t width, char* out);
/* The same under a public key of width keywidth (ProtocolElGamal.java:476-481): the plaintext group is G^keywidth, and each half
 * of a line is [width > 1: node(width; ...)] over [keywidth > 1: node(keywidth; ...)] over element trees, so
 * B = 5 + 2 ((width > 1 ? 5 : 0) + width ((keywidth > 1 ? 5 : 0) + keywidth E)) [NOT-IN-REF: PPGroupElement.toByteTree is VCR
 * code; SURVEY.md App. D's rule, applied once more].  The 2 * keywidth * width component arrays come and go in flat order, the
 * u half first, component c = l * keywidth + j the key j of plaintext component l.  keywidth = 1 is the functions above (which
 * call these); width = 1 gives the bytes of an unkeyed list of width keywidth.  Defects are reported as above; the bounds on
 * the widths are the ones above, applied to keywidth * width.  The nesting lives in the line's template and mask alone: the
 * kernels and the number of launches are those of an unkeyed list of width keywidth * width. */
size_t vmn_hexlines_line_bytes_keyed(const vmn_group* grp, size_t keywidth, size_t width);
int vmn_garrays_from_hexlines_keyed(vmn_group* grp, size_t keywidth, size_t width, const char* text, size_t len, size_t expected_n,
                                    vmn_garray** out, size_t* n_out, int* format_ok, size_t* first_bad_line, int* all_in_range);
size_t vmn_garrays_hexlines_size_keyed(const vmn_garray* const* comps, size_t keywidth, size_t width);
int vmn_garrays_to_hexlines_keyed(const vmn_garray* const* comps, size_t keywidth, size_t width, char* out);
/* Ciphertext lists and plaintexts in the reference's `json` interface (ProtocolElGamalInterfaceJSON / ...JSONDecode: the format of
 * Helios-style ballot boxes), modular groups only, as in the reference: a curve group is VMN_ERR_UNSUPPORTED.  A ciphertext line is
 * {"alpha":"A","beta":"B"} at width 1 and [{"alpha":"A1","beta":"B1"},...,{"alpha":"Aw","beta":"Bw"}] above (pair i = u_i, v_i), a
 * plaintext line "M" resp. ["M1",...,"Mw"]; every number is a decimal string as BigInteger.toString(10) writes it, every line
 * ends with \n, there are no spaces.  csrc/jsonlines_layout.h states the text; the decimal <-> binary conversion of every number
 * runs on the GPU (csrc/decimal_kernels.h), the import / export kernels of the byte trees on its result.
 * from_jsonlines has the contract of vmn_garrays_from_hexlines: out receives the 2 * width component arrays u_1..u_width,
 * v_1..v_width of *n_out elements each; *format_ok = 0, every out[] slot NULL and *first_bad_line = the zero-based index of the
 * first defective line on a format defect; a line count that differs from a non-zero expected_n is the same with
 * *first_bad_line = min(lines, expected_n); a text without lines gives 2 * width empty arrays.  Read beyond the written form:
 * lines ended as readLine ends them, the two keys in either order, spaces and tabs between tokens, leading zeros.
 * [NOT-IN-REF: a defect is a missing, duplicate, unknown or extra key, an empty number, a sign, a non-digit in a number, a
 * backslash or a byte >= 0x80, a pair count other than width, [...] at width 1 or a bare map above, anything in front of the
 * first token or behind the closing bracket, a blank line; the reference rejects the whole file without naming the line.]
 * Values >= p (however many digits they have) and zero: as vmn_garray_from_bytetree (arrays created, entries replaced,
 * *all_in_range = 0, may be NULL); subgroup membership is vmn_garray_is_member.
 * vmn_jsonlines_max_line_bytes: the longest ciphertext line the writer can produce, newline included (0 for a null group, a curve
 * group, or a width of 0 or above 65536); n times it always suffices as cap.  to_jsonlines takes 2 * width arrays, to_jsonplain
 * width arrays (decodePlaintexts); both report the bytes written in *written, write no NUL, and return VMN_ERR_ARG, writing
 * nothing, when cap is too small for this list. */
size_t vmn_jsonlines_max_line_bytes(const vmn_group* grp, size_t width);
int vmn_garrays_from_jsonlines(vmn_group* grp, size_t width, const char* text, size_t len, size_t expected_n, vmn_garray** out,
                               size_t* n_out, int* format_ok, size_t* first_bad_line, int* all_in_range);
int vmn_garrays_to_jsonlines(const vmn_garray* const* comps, size_t width, char* out, size_t cap, size_t* written);
int vmn_garrays_to_jsonplain(const vmn_garray* const* comps, size_t width, char* out, size_t cap, size_t* written);
/* Plaintexts as text: messages encoded as group elements and decoded again -- the text interface behind a session (the
 * reference ends an election with `vmnc -plain -outi native`: ProtocolElGamalInterfaceString.decodePlaintexts, :197-236; its
 * demoCiphertexts, :315-428, is built on pGroup.encode).  [NOT-IN-REF: VCR ModPGroup, safe-prime encoding; unpinned -- encode,
 * decode and getEncodeLength are VCR code; csrc/encode_layout.h states the rule built here, on integers.]
 * vmn_group_encode_length: L = floor((bits(p) - 2) / 8) - 4, the bytes one element holds (59 / 123 / 251 / 379 / 507 at 512 / 1024 /
 * 2048 / 3072 / 4096 bits), for a modular group with p = 2q + 1 and L >= 1; 0 for every other group (curves, other cofactors, a
 * null group), over which the two functions below return VMN_ERR_UNSUPPORTED.
 * An element holds be32(len) || message || zeros on L + 4 bytes as an integer v (the empty message with a 1 behind the length),
 * stored as v or p - v, whichever is a quadratic residue (one Jacobi symbol per element, on the GPU).  Decoding folds e to
 * min(e, p - e); the element is ill-formed, its message empty, when that is 2^(8 (L + 4)) or more or its length word exceeds L.
 * A message over ncomp = keywidth * width components (flat order; 1..65536) is cut into pieces of L bytes, the later components
 * holding the empty message; decoding concatenates the components' messages whatever their lengths.
 * from_textlines: a line is its bytes; lines end as Java's readLine ends them (\n, \r, \r\n once), an empty line is the empty
 * message, text behind the last terminator is a line if not empty.  out receives ncomp arrays of *n_out elements and *fits = 1;
 * when a line has more than ncomp L bytes *fits = 0, every out[] slot is NULL and *first_long_line is the zero-based index of the
 * first such line.  A text without lines gives ncomp empty arrays.
 * to_textlines: line i is the concatenated message of element i with every 0x0A and 0x0D byte removed, then \n.
 * *all_wellformed = 0 when some element was ill-formed; *all_utf8 = 0 when some line's concatenation, BEFORE the removal (Java
 * decodes, then strips), is not well-formed UTF-8 (Unicode table 3-7) -- such a line is written byte for byte [NOT-IN-REF: Java
 * substitutes U+FFFD].  Both may be NULL.  *written receives the bytes written; no NUL; VMN_ERR_ARG, writing nothing, when cap is
 * too small for these lines: a cap of n (ncomp L + 1) always suffices.  Never writes behind cap.
 * Over a curve group the same interface is vmn_ec_group_encode_length / vmn_ec_arrays_from_textlines / _to_textlines, below. */
size_t vmn_group_encode_length(const vmn_group* grp);
int vmn_garrays_from_textlines(vmn_group* grp, size_t ncomp, const char* text, size_t len, vmn_garray** out, size_t* n_out, int* fits,
                               size_t* first_long_line);
int vmn_garrays_to_textlines(const vmn_garray* const* comps, size_t ncomp, char* out, size_t cap, size_t* written, int* all_wellformed,
                             int* all_utf8);
/* The same over curve groups: a message is a point.  [NOT-IN-REF: VCR ECqPGroup; unpinned -- csrc/ec_encode_layout.h states the
 * rule built here, on integers.]
 * vmn_ec_group_encode_length: L = floor((bits(p) - 2) / 8) - 5 for the field prime p of a curve group (18 / 22 / 24 / 26 / 34 / 42 /
 * 58 / 59 at 192 / 224 / 239 / 256 / 320 / 384 / 512 / 521 bits) when that is at least 1; 0 for a modular group and a null group, over
 * which the two functions below return VMN_ERR_UNSUPPORTED.
 * A point holds T = be32(len) || message || zeros on L + 4 bytes (the empty message with a 1 behind the length) in its x coordinate:
 * x = 256 T + c with c the least counter in 0..255 for which x^3 + a x + b is a nonzero square mod p, y the smaller of the two
 * roots as integers (one Jacobi symbol per counter and one square root per point, on the GPU).  Decoding reads x alone: the point
 * is ill-formed, its message empty, when it is the point at infinity, when x >= 2^(8 (L + 5)) or when the length word of
 * floor(x / 256) exceeds L; the counter byte and y are ignored.
 * Arguments, results and contracts are those of vmn_garrays_from_textlines / _to_textlines word for word (fits and
 * first_long_line, all_wellformed and all_utf8, a cap of n (ncomp L + 1) always suffices, never a byte behind cap, nothing left
 * allocated on failure, ncomp in 1..65536).  Should no counter of the 256 fit a record (chance 2^-256), from_textlines returns
 * VMN_ERR_FORMAT and names the line in vmn_last_error(). */
size_t vmn_ec_group_encode_length(const vmn_group* grp);
int vmn_ec_arrays_from_textlines(vmn_group* grp, size_t ncomp, const char* text, size_t len, vmn_garray** out, size_t* n_out, int* fits,
                                 size_t* first_long_line);
int vmn_ec_arrays_to_textlines(const vmn_garray* const* comps, size_t ncomp, char* out, size_t cap, size_t* written, int* all_wellformed,
                               int* all_utf8);
size_t vmn_garray_size(const vmn_garray* a);
/* the group an array belongs to (PGroupElementArray.getPGroup(), PRingElementArray.getPRing()): a binding sizes the host
 * buffers of vmn_*_to_be / _get / _prod ... from it (jni/: every byte[] is checked against the bytes the callee touches) */
vmn_group* vmn_garray_group(const vmn_garray* a);
vmn_group* vmn_rarray_group(const vmn_rarray* a);
void vmn_garray_free(vmn_garray* a);                   /* PGroupElementArray.free() */

/* K1a  X.exp(E): out[i] = X[i]^E[i].  ref: P/hvzk/PoSBasicTW.java:1032; P/hvzk/PoSCBasicTW.java:694.
 * ebits = bit length bound of the exponents actually used (<= 8*exp_bytes; 0 = full width). */
int vmn_garray_exp_array(const vmn_garray* x, const vmn_rarray* e, int ebits, vmn_garray** out);
/* Same with integer exponents that are NOT reduced mod q (LargeIntegerArray, e.g. the
 * n_e+n_v+n_r-bit k_E):  exps_be = n big-endian values of ebytes each. */
int vmn_garray_exp_ints(const vmn_garray* x, const uint8_t* exps_be, size_t ebytes, int ebits, vmn_garray** out);
/* K1b  X.exp(e) with one shared exponent.  ref: P/hvzk/PoSBasicTW.java:1028;
 * P/mixnet/ShufflerElGamalSession.java:506; P/mixnet/PermutationCommitment.java:357;
 * P/elgamal/DistrElGamalSession.java:384-385. */
int vmn_garray_exp_scalar(const vmn_garray* x, const uint8_t* e_be, size_t ebytes, vmn_garray** out);
/* The same for k arrays of one group and one size under ONE exponent: outs[c][i] = xs[c][i]^e, bit for bit what k calls of
 * vmn_garray_exp_scalar give (the omega component arrays of a width-omega list raised to a party's secret:
 * P/elgamal/DistrElGamalSession.java:365-389 over a product group).  Over a modular group, for exponents above 32 bits, up to
 * eight arrays share one launch; VMN_EXP_MULTI_FUSED=0 (read per call) runs them one after the other.  Over a curve up to
 * eight arrays share one launch as well, whatever the scalar: it is reduced modulo the group order and recoded into signed odd
 * digits on the host (VMN_EC_SHARED=0, read per call: the fixed-window kernel for per-point scalars, array by array).  The same
 * array may appear twice.  k = 0, arrays of two groups or of different sizes: VMN_ERR_ARG.  On failure no output stays allocated
 * (outs[c] = NULL). */
int vmn_garray_exp_scalar_multi(const vmn_garray* const* xs, size_t k, const uint8_t* e_be, size_t ebytes, vmn_garray** outs);
/* The same with an exponent per ARRAY: outs[c][i] = xs[c][i]^(e_c), es_be holds k rows of ebytes bytes, row c the exponent of
 * array c; bit for bit what vmn_garray_exp_scalar gives for (xs[c], e_c).  Under a public key of width kappa the component
 * arrays of a party's decryption factors take kappa different secrets (P/elgamal/DistrElGamalSession.java:365-389 over
 * (G^kappa)^omega).  Over a modular group with every exponent above 32 bits up to eight arrays share one launch, each under a
 * schedule of its own; VMN_EXP_MULTI_FUSED=0 (read per call) runs them one after the other.  Over a curve up to eight arrays
 * share one launch, each under the schedule of its own scalar, zero included (VMN_EC_SHARED=0: array by array, as before).  Over
 * a modular group with any exponent of at most 32 bits in the call, the arrays run one after the other, each as
 * vmn_garray_exp_scalar runs it.  Arguments and failures as for vmn_garray_exp_scalar_multi. */
int vmn_garray_exp_scalars_multi(const vmn_garray* const* xs, size_t k, const uint8_t* es_be, size_t ebytes, vmn_garray** outs);
/* K2  g.exp(E): out[i] = base^E[i] for one fixed base.  ref: P/mixnet/ShufflerElGamalSession.java:407,
 * 658; P/hvzk/PoSBasicTW.java:447, 606, 608, 644, 646, 1030; P/mixnet/PermutationCommitment.java:200. */
int vmn_group_exp_fixed(vmn_group* grp, const uint8_t* base_be, const vmn_rarray* e, vmn_garray** out);
/* Session setup: build the fixed-base table of a long-lived base (the generator, the public key) for arrays of about
 * n_hint exponents and about uses_hint calls.  The window is the one that is best over those uses (w = 19 = a 17 GB
 * table at 2048 bits, N = 10^6, instead of w = 16 = 2.5 GB for a base seen once: 108 instead of 128 products per
 * exponentiation); allocating it takes ~0.6 s, which is why it belongs to setup.  VCR precomputes fixed-base tables
 * the same way when it is handed a generator it will exponentiate many times.  Bases that are never announced get
 * the one-call window on first use. */
int vmn_group_precompute_fixed(vmn_group* grp, const uint8_t* base_be, size_t n_hint, int uses_hint);
/* The table of a base that will not be used again (a prover's per-proof base h_0 when the proof object is freed -- the
 * reference frees a proof's arrays in PoSBasicTW.free(), P/hvzk/PoSBasicTW.java:1088-1101; VCR keeps no table beyond a call):
 * it leaves the group's cache and its memory serves the next table of that size.  Unknown base: no effect. */
int vmn_group_release_fixed(vmn_group* grp, const uint8_t* base_be);
/* K3  X.expProd(E) = prod_i X[i]^E[i] -> one element (big-endian, elem_bytes).
 * ref: P/hvzk/PoSBasicTW.java:408, 409, 481, 690, 1021, 1063; P/hvzk/CCPoSBasicW.java:380, 391, 497-503. */
int vmn_garray_expprod(const vmn_garray* x, const vmn_rarray* e, int ebits, uint8_t* out_be);
int vmn_garray_expprod_ints(const vmn_garray* x, const uint8_t* exps_be, size_t ebytes, int ebits, uint8_t* out_be);
/* The same for k arrays under ONE exponent array (the 2*width component arrays of a ciphertext array:
 * PPGroupElementArray.expProd, ref: P/hvzk/PoSBasicTW.java:409, 690, 1063; P/hvzk/CCPoSBasicW.java:391, 498, 567):
 * the exponent digits are sorted once; out_be receives k elements. */
int vmn_garray_expprod_multi(const vmn_garray* const* xs, size_t k, const vmn_rarray* e, int ebits, uint8_t* out_be);
/* The same in two halves.  _begin queues the device part and returns a handle; vmn_pending_finish waits for it, completes
 * the k elements into out_be and releases the handle (also when it fails); vmn_pending_free abandons a handle that is not
 * finished.  Between the two the caller queues its other device work: the tail of a multi-exponentiation over a modular
 * group is a chain of squarings on the host (one per exponent bit), during which the device would otherwise have nothing
 * to do -- at the reference's demo size (10^4 ciphertexts) a tenth of a proof.  The arrays must stay alive until finish. */
typedef struct vmn_pending vmn_pending;
int vmn_garray_expprod_multi_begin(const vmn_garray* const* xs, size_t k, const vmn_rarray* e, int ebits, vmn_pending** out);
int vmn_pending_finish(vmn_pending* p, uint8_t* out_be);
size_t vmn_pending_bytes(const vmn_pending* p);   /* what finish writes: k elements */
void vmn_pending_free(vmn_pending* p);
/* K3'  pGroup.expProd(bases[], integers[], bitLength): out[i] = prod_j xs[j][i]^(c_j), c_j = (negative[j] ? -1 : 1) * abs_j, the
 * c_j the same for every position.  ref: P/elgamal/DistrElGamalSessionBasic.java:465-503 (the modified Lagrange integers of
 * combineDecryptionFactors); with the second ciphertext components v as one more base under exponent 1 the same call recovers
 * the plaintexts, v * prod_j f_j^(lambda_j) (P/mixnet/MixNetElGamalVerifyFiatShamirSession.java:1268-1273).
 * abs_be: k rows of ebytes big-endian bytes (the layout vmn_lagrange_coefficients writes); bitlen = bound on bits(abs_j),
 * 0 = 8*ebytes.  The integers are not reduced modulo the group order by the caller (over a curve the library reduces them).
 * One chain of squarings (doublings) serves all bases, up to eight bases per launch; over a modular group the positive and the
 * negative part are two products of one launch and the negative one goes through vmn_garray_inv, over a curve a negative
 * coefficient negates its base.  The result is bit for bit what vmn_garray_exp_scalar, _mul and _inv give.  An exponent 0 drops
 * its base; all exponents 0: the array of ones (of infinity).  The same array may appear more than once.  k = 0, arrays of two
 * groups or sizes, an abs_j of more than bitlen bits, bitlen > 8*ebytes, over a modular group arrays of 2^31 elements or more:
 * VMN_ERR_ARG, *out is not written. */
int vmn_garray_expprod_arrays(const vmn_garray* const* xs, size_t k, const uint8_t* abs_be, size_t ebytes, const int* negative,
                              int bitlen, vmn_garray** out);
/* K4  X.mul(Y).  ref: P/mixnet/ShufflerElGamalSession.java:273, 789, 850 (the re-encryption);
 * P/hvzk/PoSBasicTW.java:448, 610, 648, 1029, 1033. */
int vmn_garray_mul(const vmn_garray* x, const vmn_garray* y, vmn_garray** out);
/* Element-wise inverse X.inv() by Montgomery's batch inversion (two product scans + one host inversion
 * of the total + 2N products instead of N exponentiations).  Serves the negative modified Lagrange
 * coefficients of pGroup.expProd(bases[], integers[], bitLength),
 * ref: P/elgamal/DistrElGamalSessionBasic.java:487-502 (K3'), :406-452 (coefficients may be negative). */
int vmn_garray_inv(const vmn_garray* x, vmn_garray** out);
/* out[i] = x[i]^e * y[i]^f[i] as ONE simultaneous power: the squarings are shared between the two exponents
 * (max(bits(e), fbits) of them instead of the sum).  Curves: one chain of doublings for the two scalar multiplications
 * (e acts through its residue modulo the group order).  The
 * verifiers' check (B) of PoSBasicTW.java:1023-1042 in the form B_i^v (B_{i-1}^{-1})^{k_E,i} B'_i = g^{k_B,i}. */
int vmn_garray_exp2(const vmn_garray* x, const uint8_t* e_be, size_t ebytes, const vmn_garray* y, const vmn_rarray* f, int fbits,
                    vmn_garray** out);
/* out_x[i] = x[i]^e and out_y[i] = y[i]^f[i], the two powers of the same check in its separate form
 * (PoSBasicTW.java:1028-1033: B.exp(v) and B_shift.exp(k_E)), as ONE launch when the arrays are too small to fill
 * the device one after the other; otherwise (and over curves, where the shared half takes the signed windows of
 * vmn_garray_exp_scalar) exactly vmn_garray_exp_scalar + vmn_garray_exp_array.
 * x and y may differ in length; f has y's. */
int vmn_garray_exp_pair(const vmn_garray* x, const uint8_t* e_be, size_t ebytes, const vmn_garray* y, const vmn_rarray* f, int fbits,
                        vmn_garray** out_x, vmn_garray** out_y);
/* K5  X.prod() -> one element.  ref: P/hvzk/PoSBasicTW.java:1013; P/hvzk/PoSCBasicTW.java:667. */
int vmn_garray_prod(const vmn_garray* x, uint8_t* out_be);
/* K6  X.equals(Y).  ref: P/hvzk/PoSBasicTW.java:1035; P/hvzk/PoSCBasicTW.java:697. */
int vmn_garray_equals(const vmn_garray* x, const vmn_garray* y, int* equal);
/* K7  data movement.  permute: out[i] = X[perm[i]] (gather; see SURVEY.md App. B on the convention);
 * shiftPush: (el, X[0..n-2]); copyOfRange [from, to); extract keeps X[i] where keep[i] != 0.
 * ref: P/mixnet/ShufflerElGamalSession.java:278, 684-703, 792; P/hvzk/PoSBasicTW.java:451, 637-638, 1031;
 * P/mixnet/PermutationCommitment.java:398-405, 462-469. */
int vmn_garray_permute(const vmn_garray* x, const uint32_t* perm_host, vmn_garray** out);
/* General gather: out[i] = X[idx[i]], i < n_out (n_out may differ from the array's size: a shard of a
 * permuted array is a gather of the replicated input). */
int vmn_garray_gather(const vmn_garray* x, const uint32_t* idx_host, size_t n_out, vmn_garray** out);
int vmn_garray_shift_push(const vmn_garray* x, const uint8_t* el_be, vmn_garray** out);
int vmn_garray_copy_range(const vmn_garray* x, size_t from, size_t to, vmn_garray** out);
int vmn_garray_extract(const vmn_garray* x, const uint8_t* keep_host, vmn_garray** out);
int vmn_garray_get(const vmn_garray* x, size_t i, uint8_t* out_be);
/* pGroup.toElementArray(PGroupElementArray[]) and copyOfRange in one: out holds the rows [from[k], to[k]) of src[k], k = 0 .. nseg-1,
 * one segment after the other.  Segments may be empty, may overlap, and one array may be named more than once; the sources are
 * read only.  nseg == 0 gives the empty array of grp.  VMN_ERR_ARG and no array (*out = NULL) for a null argument, a source of
 * another group, from[k] > to[k], to[k] > the size of src[k], nseg > 65536, or a row total that overflows.  One launch per call
 * whatever nseg is (csrc/light_kernels.h k_rows_segments), also for one segment.
 * ref: ProtocolElGamalRear.java:430-473, ProtocolElGamalInterfaceSeq.java:181. */
int vmn_garray_from_segments(vmn_group* grp, const vmn_garray* const* src, const size_t* from, const size_t* to, size_t nseg,
                             vmn_garray** out);
/* Subgroup membership of every element; *all_members = 1/0.  Part of K10 (the check pGroup.toElementArray makes
 * when an array is read).  Safe-prime groups up to 3072 bits: Jacobi symbol (x / p) = 1 by the binary algorithm,
 * one element per lane (10^6 elements in 46 ms); otherwise x^q = 1 (749 ms); curves: the import's on-curve check
 * already is the membership test (cofactor 1). */
int vmn_garray_is_member(const vmn_garray* x, int* all_members);

/* ---- ring element arrays over Z_q (PRingElementArray / PFieldElementArray) ------------------ */

int vmn_rarray_from_be(vmn_group* grp, const uint8_t* be, size_t n, vmn_rarray** out, int* all_in_range);
int vmn_rarray_to_be(const vmn_rarray* a, uint8_t* be_out);
size_t vmn_rarray_size(const vmn_rarray* a);
void vmn_rarray_free(vmn_rarray* a);
/* K8.  ref: P/hvzk/PoSBasicTW.java:596 (recLin), 604 (prods), 642-645, 861-863, 873-878, 1014;
 * P/hvzk/PoSCBasicTW.java:410, 418, 483-486, 612-613, 623-627, 668; P/hvzk/CCPoSBasicW.java:467-478. */
int vmn_rarray_mul(const vmn_rarray* x, const vmn_rarray* y, vmn_rarray** out);
int vmn_rarray_add(const vmn_rarray* x, const vmn_rarray* y, vmn_rarray** out);
int vmn_rarray_neg(const vmn_rarray* x, vmn_rarray** out);
/* x.mulAdd(v, y): out[i] = x[i]*v + y[i] with scalar v (big-endian, exp_bytes); y == NULL: out[i] = x[i]*v. */
int vmn_rarray_mul_add(const vmn_rarray* x, const uint8_t* v_be, const vmn_rarray* y, vmn_rarray** out);
/* b.recLin(e): x[0] = b[0], x[i] = x[i-1]*e[i] + b[i]; last = x[n-1] (may be NULL). */
int vmn_rarray_rec_lin(const vmn_rarray* b, const vmn_rarray* e, vmn_rarray** out_x, uint8_t* last_be);
/* e.prods(): y[i] = prod_{j<=i} e[j]. */
int vmn_rarray_prods(const vmn_rarray* e, vmn_rarray** out);
int vmn_rarray_inner_product(const vmn_rarray* x, const vmn_rarray* y, uint8_t* out_be);
int vmn_rarray_sum(const vmn_rarray* x, uint8_t* out_be);
/* k of those in ONE round trip: out_be[i] = <xs[i], ys[i]>, or the sum of xs[i] where ys[i] is NULL (a reply's <r, e'>,
 * sum r and <s_c, e>, ref: P/hvzk/PoSBasicTW.java:856-888).  out_be receives k ring elements. */
int vmn_rarray_inner_products(const vmn_rarray* const* xs, const vmn_rarray* const* ys, size_t k, uint8_t* out_be);
int vmn_rarray_prod(const vmn_rarray* x, uint8_t* out_be);
int vmn_rarray_permute(const vmn_rarray* x, const uint32_t* perm_host, vmn_rarray** out);
int vmn_rarray_gather(const vmn_rarray* x, const uint32_t* idx_host, size_t n_out, vmn_rarray** out);
int vmn_rarray_shift_push(const vmn_rarray* x, const uint8_t* el_be, vmn_rarray** out);
int vmn_rarray_equals(const vmn_rarray* x, const vmn_rarray* y, int* equal);
int vmn_rarray_get(const vmn_rarray* x, size_t i, uint8_t* out_be);
int vmn_rarray_copy_range(const vmn_rarray* x, size_t from, size_t to, vmn_rarray** out);
/* Largest bit length among the entries (0 for an empty or all-zero array).  A verifier must use EVERY bit of an
 * exponent array it received (pField.toElementArray parses full field elements, ref: P/hvzk/PoSBasicTW.java:985-989, and
 * h.expProd(k_E) :1021, B_shift.exp(k_E) :1032 use them whole); this tells it how many there are, so that honest
 * replies (n_e + n_v + n_r + 1 bits) keep their short exponentiations and anything longer is still computed exactly. */
int vmn_rarray_max_bits(const vmn_rarray* x, int* bits);

/* ---- pseudo-random derivations ---------------------------------------------
 * VCR's PRGHeuristic and RandomOracle over SHA-256 / SHA-384 / SHA-512 (the three the reference offers,
 * ref: P/elgamal/ProtocolElGamal.java:352-371 PRG, :413-434 random-oracle hash), restated from their published definition
 * (the classes are not in the reference tree): PRG(seed) = H(seed || uint32_be(0)) || H(seed || uint32_be(1)) || ...;
 * RO_nout(d) = first ceil(nout/8) bytes of PRG(H(uint32_be(nout) || d)) with the superfluous leading bits cleared.
 * A PRG seed has the digest's length (PRGHeuristic.minNoSeedBytes), so seedlen = 32 / 48 / 64 selects the hash everywhere
 * a seed is taken.  The SHA-256 constructions are pinned by the published known-answer vectors, SHA-384 / SHA-512 by
 * hashlib (tests/test_prg.py). */
int vmn_prg_bytes(const uint8_t* seed, size_t seedlen, uint8_t* out, size_t nbytes);              /* host */
int vmn_random_oracle(const uint8_t* data, size_t len, int nout_bits, uint8_t* out);            /* host, SHA-256 */
int vmn_random_oracle_hash(int hash_bits, const uint8_t* data, size_t len, int nout_bits, uint8_t* out);   /* 256 / 384 / 512 */
/* The random vector of a proof, generated on the device: prg.setSeed(seed); LargeIntegerArray.random(n, bits, prg)
 * as field elements.  ref: P/hvzk/PoSBasicTW.java:533-538, PoSCBasicTW.java:350-355, CCPoSBasicW.java:330-335.
 * Value i = the i-th ceil(bits/8) bytes of the stream, leading bits cleared; reduced mod q when it can reach q. */
int vmn_rarray_from_prg(vmn_group* grp, const uint8_t* seed, size_t seedlen, size_t n, int bits, vmn_rarray** out);
/* Parts of the same array without the rest (the stream is counter mode): values [first, first + n), resp. the values
 * idx[0 .. n-1] (host indices) -- equal to copy_range / gather of vmn_rarray_from_prg(.., N, ..).  A rank of a sharded
 * proof generates its own positions of r, s, b, beta, epsilon, e and the rows e_{pi^-1(i)}, r_{pi(i)}, s_{pi^-1(i)} it
 * reads through the permutation, instead of all N values on every GPU (the reference has no counterpart:
 * P/hvzk/PoSBasicTW.java:446, 473, 552-554 run on one machine). */
int vmn_rarray_from_prg_range(vmn_group* grp, const uint8_t* seed, size_t seedlen, size_t first, size_t n, int bits, vmn_rarray** out);
int vmn_rarray_from_prg_gather(vmn_group* grp, const uint8_t* seed, size_t seedlen, const uint32_t* idx, size_t n, int bits,
                               vmn_rarray** out);
/* A prover's secret permutation, drawn on the device: Permutation.random(size, randomSource, rbitlen) of
 * mixnet/ShufflerElGamalSession.java:408-409 and mixnet/PermutationCommitment.java:209 [NOT-IN-REF: VCR Permutation.random;
 * unpinned -- the rule is stated in csrc/permutation_layout.h].  Key i = the i-th key_bytes bytes of PRG(seed), leading bits
 * cleared (vmn_rarray_from_prg's convention), with kb = rbitlen + 2 ceil(log2(max(n, 2))) key bits and key_bytes = ceil(kb / 8);
 * pi[j] = the index of rank j in the order (key, index), inv[pi[j]] = j.  Within 2^-rbitlen of uniform.  n < 2^32 (n = 0 and 1
 * are valid), rbitlen 0 .. 256.  The sort is a radix sort of the indices on the device (csrc/permutation_kernels.h), exact and
 * the same bytes on every run and every rank; the tables come back as HOST tables, which is what every entry point that takes
 * `const uint32_t* pi` expects.  Either table may be NULL, not both.  Bad arguments: VMN_ERR_ARG, nothing written. */
size_t vmn_permutation_key_bytes(size_t n, int rbitlen);               /* 0 when the arguments are out of range */
/* the same order for keys the caller holds: n big-endian rows of key_bytes bytes (1 .. 64) */
int vmn_permutation_from_keys(vmn_ctx* ctx, const uint8_t* keys_be, size_t key_bytes, size_t n, uint32_t* pi_out, uint32_t* inv_out);
int vmn_permutation_from_prg(vmn_ctx* ctx, const uint8_t* seed, size_t seedlen, size_t n, int rbitlen, uint32_t* pi_out,
                             uint32_t* inv_out);
/* Independent generators: pGroup.randomElementArray(n, prg, rbitlen) of a ModPGroup, generated on the
 * device.  ref: P/distr/IndependentGeneratorsRO.java:117-130 (seed = RO(globalPrefix || bytetree(sid))).
 * t_i = the i-th ceil((bits(p) + rbitlen)/8) bytes, leading bits cleared; h_i = t_i^((p-1)/q) mod p -- a squaring for
 * the safe-prime groups the reference generates, a power with the group's own cofactor otherwise (the reference's
 * ModPGroup_1024_256, demo/mixnet/group_descriptions:29; tests/test_bytetree.py).
 * ECqPGroup (P-256 is the reference's default group, demo/mixnet/.conf:153): the values are candidates for x = t mod p,
 * kept when x^3 - 3x + b is a square, with the smaller root as y; element i is the i-th kept candidate (candidates are
 * tested in parallel, the kept ones compacted in order).
 * The derivations follow the specification's text; they are not pinned by a vector of the reference [NOT-IN-REF]. */
int vmn_garray_from_prg(vmn_group* grp, const uint8_t* seed, size_t seedlen, size_t n, int rbitlen, vmn_garray** out);

/* ---- partial results for multi-GPU sharding --------------------------------
 * Each rank holds a contiguous shard; expProd/prod partials are single elements that the host
 * side exchanges (RCCL all-gather of G x elem_bytes) and multiplies.  This multiplies k partials
 * given as k*elem_bytes big-endian bytes into one element. */
int vmn_group_mul_partials(vmn_group* grp, const uint8_t* partials_be, size_t k, uint8_t* out_be);

/* ---- instrumentation ---------------------------------------------------------------------- */
/* Name, launch count and accumulated device time (ms, HIP events on the context stream) of the
 * kernel families since the last reset; used by bench.py for the roofline line.  Timing is off
 * by default (no events recorded). */
int vmn_ctx_timing_enable(vmn_ctx* ctx, int on);
int vmn_ctx_timing_reset(vmn_ctx* ctx);
/* family: "modpow", "modmul", "fixed", "expprod", ...; returns launches and total ms. */
int vmn_ctx_timing_get(vmn_ctx* ctx, const char* family, long* launches, double* total_ms);
/* All families as text lines "family launches total_ms executed_mads canonical_macs\n" into buf (truncated to len-1 bytes):
 * executed_mads = v_mad_u64_u32 multiply-adds of the 28-bit-limb kernels, canonical_macs = the same products priced at
 * SURVEY.md 8d's M(s) = 2 s^2 + s / Q(s) on s = bits / 32 limbs (the unit of the headline roofline). */
int vmn_ctx_timing_report(vmn_ctx* ctx, char* buf, size_t len);

#ifdef __cplusplus
}
#endif
#endif /* VMNHIP_H */
