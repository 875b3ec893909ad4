/*
 * libstarkperp - C ABI of the MI355X hot path for the StarkEx-Perpetual crypto builtins.
 *
 * The reference (starkware-libs/stark-perpetual) has no FFI: its hot path is the Python module
 * src/starkware/crypto/signature/signature.py.  Each entry point below names the reference
 * function (file:line, relative to /root/reference/src) whose arithmetic it replaces; the Python
 * host package (stark-perpetual_amd/starkperp) binds them with ctypes and re-exposes the
 * reference's module API unchanged.  INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - A field element / scalar ("felt") is 32 bytes: four little-endian uint64 limbs, plain
 *     (non-Montgomery) integer value.  Arrays are contiguous, n * 32 bytes, caller-owned.
 *   - Functions ending in _dev take DEVICE pointers (HBM resident, 32-byte aligned) and a
 *     hipStream_t passed as void* (NULL = the null stream); they enqueue work and return without
 *     synchronising.  The others take HOST pointers and are synchronous.
 *   - Return value: 0 on success, negative on library/runtime error (sp_last_error() has the
 *     text).  Data-dependent outcomes are reported per item in a uint8_t status array.
 *   - There is no CPU fallback: without a visible gfx950 device sp_init fails and every compute
 *     entry point returns SP_ERR_NOT_INITIALISED.
 *   - Ownership: the library never keeps a caller pointer after a host-pointer call returns; a _dev
 *     call's buffers must stay valid until the work enqueued on its stream has completed.
 *   - Threading: every entry point may be called from any host thread.  One recursive lock
 *     serialises the host-side bookkeeping; scratch, window tables of the verifier and NTT work
 *     columns are per stream, so _dev calls on different streams overlap on the device.  Every
 *     host-pointer batch runs on one of 16 host lanes (own stream, own staging buffers), makes one round trip on
 *     that stream - no device-wide wait - and holds the lock only while it enqueues: calls from different threads
 *     overlap on the device - on the devices, after sp_init_devices - (a seventeenth concurrent caller waits for a
 *     lane).  Keyed verification holds the lock to register keys and to enqueue; a persistent tree has its own
 *     stream and mutex (below).  The exceptions, which hold the lock from start to end: key registration
 *     (sp_ecdsa_register_keys), sp_ecdsa_key_cache_reset, sp_init and sp_init_devices.
 *     A lane's device buffer only grows until sp_shutdown: one huge sp_merkle_root or sp_pedersen_batch leaves its
 *     buffer parked on the lane that served it.
 *     Each entry point binds the device given to sp_init for its duration and restores the calling
 *     thread's current HIP device on return.
 */
#ifndef STARKPERP_H
#define STARKPERP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SP_OK 0
#define SP_ERR_NOT_INITIALISED (-1)
#define SP_ERR_HIP (-2)
#define SP_ERR_BAD_ARGUMENT (-3)
#define SP_ERR_TABLE_BUILD (-4)
#define SP_ERR_CACHE_FULL (-5) /* sp_ecdsa_register_keys: no free key-table slot */

/* per-item status of sp_pedersen_* (signature.py:300-318).  sp_pedersen_batch[_dev] write status[i] for every
 * item, exactly: SP_HASH_OUT_OF_RANGE for item i if and only if x[i] or y[i] is not in [0, p), whatever n is and
 * wherever in the batch the item sits; the items around it are hashed as usual.  out[i] of an item whose status is
 * not SP_HASH_OK is unspecified (the kernels differ in what they leave there): read status[i] before out[i]. */
#define SP_HASH_OK 0
#define SP_HASH_OUT_OF_RANGE 1 /* an input was not in [0, p): signature.py:307 assertion; out[i] is unspecified */
#define SP_HASH_UNHASHABLE 2   /* exceptional point collision: signature.py:313 ("Unhashable input.") */
#define SP_TREE_NOT_COMMITTED 0x80 /* sp_order_batch: a signature did not verify - the tree was left as it was */

/* per-item result of sp_ecdsa_verify_* (signature.py:217-260) */
#define SP_VERIFY_FALSE 0
#define SP_VERIFY_TRUE 1
#define SP_VERIFY_ASSERT_S 2     /* signature.py:219  assert 1 <= s < EC_ORDER */
#define SP_VERIFY_ASSERT_R 3     /* signature.py:225  assert 1 <= r < 2**251 */
#define SP_VERIFY_ASSERT_W 4     /* signature.py:226  assert 1 <= w < 2**251 */
#define SP_VERIFY_ASSERT_MSG 5   /* signature.py:227  assert 0 <= msg_hash < 2**251 */
#define SP_VERIFY_ASSERT_CURVE 6 /* signature.py:241  assert is_point_on_curve */
#define SP_VERIFY_STALE_SLOT 7   /* sp_ecdsa_verify_keyed_dev only: the slot handle is not from the current
                                    cache generation (handed out before sp_ecdsa_key_cache_reset) or was never
                                    handed out; no verdict was computed for this item */

/* per-item status of sp_ecdsa_sign_* (signature.py:137-173) */
#define SP_SIGN_OK 0
#define SP_SIGN_RETRY 1          /* the k was rejected (signature.py:158-170): draw the next k */
#define SP_SIGN_BAD_INPUT 2      /* msg_hash >= 2**251 (signature.py:141) or key/k out of range */

/* ---- lifecycle ---------------------------------------------------------------------------- */
/* Selects the HIP device and builds the window tables of the Pedersen constant points
 * (signature.py:43 CONSTANT_POINTS; table structure nothing_up_my_sleeve_gen.py:88-90) and of
 * EC_GEN (signature.py:56) in HBM.  window_bits = 0 picks the default (21: 2^20 + 22 x 2^21 Pedersen entries + 12 x 2^21
 * EC_GEN entries, 64 B each = 4.3 GiB of tables; 26 = 75 GiB, 19 entries per hash, ~15 % faster hashing: what the
 * benchmark runs with).  The first sp_init of a process also runs 64 asynchronous 128-KiB copies each way (~8 ms):
 * the HIP runtime takes a one-time 6 - 7 ms step at about the 43rd sizeable copy of a process, which would
 * otherwise land inside a caller's batch (STARKPERP_NO_COPY_WARMUP=1 skips it).  Idempotent. */
int sp_init(int device, int window_bits);
/* Several devices in one process (the SURVEY 8(b) shape `sp_init(n_devices, device_ids)`): one context - its own
 * window tables - per entry of device_ids; context 0 is the PRIMARY.  What runs where:
 *   - the stateless batches run on ANY context: sp_pedersen_batch, sp_ecdsa_verify_batch (ladder),
 *     sp_ecdsa_sign_batch, sp_ecdsa_sign_rfc6979_batch, sp_public_key_batch, sp_felt_sqrt_batch,
 *     sp_stark_key_y_batch, sp_ec_mult_batch, sp_ec_lincomb_batch, sp_ec_add_batch take the context of the host lane
 *     they are handed (lanes go round-robin over the contexts, so concurrent host threads spread over the
 *     devices), and one call of sp_pedersen_batch / sp_ecdsa_verify_batch with 16384 items or more is cut into
 *     one contiguous slice per context, the slices running side by side on host threads of the library; sp_pedersen_batch_dev, sp_pedersen_chains_dev, sp_pedersen_chains_ragged_dev, sp_merkle_fold_paths_dev, sp_merkle_build_dev, sp_merkle_forest_dev,
 *     sp_commit_rows_dev, sp_ecdsa_verify_batch_dev, sp_ecdsa_sign_batch_dev, sp_ecdsa_sign_rfc6979_batch_dev,
 *     sp_public_key_batch_dev, sp_felt_sqrt_batch_dev, sp_stark_key_y_batch_dev, sp_ec_mult_batch_dev,
 *     sp_ec_lincomb_batch_dev, sp_ec_add_batch_dev and sp_commit_open_dev (sp_commit_open too: its tables are
 *     device pointers) run on the device their pointers
 *     live on (the stream
 *     must belong to that device);
 *   - everything with state - persistent trees, key tables, the prover entry points (twiddle tables, witness
 *     scratch) and the remaining host-pointer calls - stays on the primary device.
 * The reference's deployment model here is one process per GPU (torch.distributed ranks, bench.py); this
 * entry point is for a C caller that drives a node from one process.  Idempotent for the same layout;
 * another layout needs sp_shutdown first.  A device may be listed twice (two contexts on one GPU: tests). */
int sp_init_devices(int n_devices, const int* device_ids, int window_bits);
int sp_device_count(void);  /* contexts initialised (0 before sp_init) */
/* device index and host-lane calls served so far by context `index` */
int sp_context_info(int index, int* device, uint64_t* host_calls);
void sp_shutdown(void);
const char* sp_last_error(void);
int sp_is_initialised(void);
/* window width in use and bytes of HBM held by the tables */
int sp_window_bits(void);
size_t sp_table_bytes(void);
int sp_synchronize(void* stream);
/* Build provenance (no reference counterpart: the reference is interpreted Python): one static line naming the
 * compiler, the HIP version, the offload architecture, the compile date of the library and the sanitizer it was
 * instrumented with, if any - bench.py prints it next to the sha256 of the .so, so that the binary a record was
 * produced by can be identified.  Callable before sp_init. */
const char* sp_build_info(void);

/* Measurement aid: between sp_profile_begin and sp_profile_end every launch of the dominant kernel
 * (ped_accumulate_kernel) is bracketed by HIP events on the stream it is launched on; _end returns
 * the summed kernel time, the number of launches and the number of hashes they processed.  The launches of
 * sp_felt_sqrt_batch*, sp_stark_key_y_batch* and the three sp_ec_*_batch* calls are bracketed the same way (units:
 * items), and so are those of sp_commit_open* (units: openings). */
int sp_profile_begin(size_t max_launches);
int sp_profile_end(double* total_ms, uint64_t* launches, uint64_t* units);

/* ---- Pedersen hash: pedersen_hash(x, y) signature.py:296-318 -------------------------------- */
int sp_pedersen_batch(const uint64_t* x, const uint64_t* y, uint64_t* out, uint8_t* status, size_t n);
int sp_pedersen_batch_dev(const uint64_t* x, const uint64_t* y, uint64_t* out, uint8_t* status,
                          size_t n, void* stream);
/* pedersen_hash_as_point(x, y) signature.py:300-318: the full affine point (testing helper). */
int sp_pedersen_point_batch(const uint64_t* x, const uint64_t* y, uint64_t* out_x, uint64_t* out_y,
                            uint8_t* status, size_t n);
/* left fold h = H(h, e_i) starting from h = e_0: the hash-chain shape of
 * perpetual_messages.py:279-286 and position/hash.cairo:22-43.  n_elems >= 1. */
int sp_pedersen_chain(const uint64_t* elems, size_t n_elems, uint64_t* out, uint8_t* status);
/* right fold h = H(e_i, h) starting from h = e_{n-1}: cairo-lang compute_hash_chain, the consumer
 * behind starkware/cairo/bootloaders/program_hash_test_utils.py:9. */
int sp_pedersen_chain_right(const uint64_t* elems, size_t n_elems, uint64_t* out, uint8_t* status);
/* width independent chains of equal depth, element j of chain i at elems[(j*width + i)*4]:
 * out[i] = H(...H(H(e0,e1),e2)...,e_{depth-1}) */
int sp_pedersen_chains_dev(const uint64_t* elems, size_t width, size_t depth, uint64_t* out,
                           uint8_t* status, void* stream);
/* same with host pointers (status: OR of the item status bytes) */
int sp_pedersen_chains(const uint64_t* elems, size_t width, size_t depth, uint64_t* out, uint8_t* status);
/* n independent left-fold chains of unequal length, chain-major: chain i = elems[4*off[i] .. 4*off[i+1]),
 * off = n + 1 HOST offsets in felts, off[0] = 0, non-decreasing by >= 1.  out: n felts.  status: n bytes or NULL.
 * out[i] = H(...H(H(e0,e1),e2)...,e_{len-1}), the element itself for a chain of one; status[i] = OR of the status
 * bytes of chain i's hashes (SP_HASH_OUT_OF_RANGE also for the only word of a one-word chain).  The message hashes
 * of a mixed transaction batch (execute_batch.cairo:296-343: chains of 2 to 6 words) and position leaves of
 * different asset counts (position/hash.cairo:22-74) in ONE launch that lasts as long as its longest chain; batches
 * above the largest launch class (8192 chains) go out as consecutive slices on the same stream.  A zero-length
 * chain or off[0] != 0: SP_ERR_BAD_ARGUMENT, nothing is written.  The _dev call enqueues and returns; it has
 * copied `off` by then. */
int sp_pedersen_chains_ragged_dev(const uint64_t* elems, const uint32_t* off, size_t n,
                                  uint64_t* out, uint8_t* status, void* stream);   /* elems/out/status on the device */
int sp_pedersen_chains_ragged(const uint64_t* elems, const uint32_t* off, size_t n,
                              uint64_t* out, uint8_t* status);                     /* all host pointers, runs on a host lane */

/* ---- Merkle trees with node = pedersen_hash(left, right) ------------------------------------- */
/* (merkle_multi_update call sites services/perpetual/cairo/state/state.cairo:155-173)           */
/* Full rebuild over 2^height leaves.  levels_out (optional, may be NULL) receives every level
 * bottom-up, leaves first: (2^(height+1) - 1) felts.  status is a single byte (OR of item status). */
int sp_merkle_root(const uint64_t* leaves, unsigned height, uint64_t* root, uint64_t* levels_out,
                   uint8_t* status);
/* Device version: `levels` is a device buffer of (2^(height+1) - 1) felts whose first 2^height
 * entries hold the leaves; the upper levels are written behind them, the root last. */
int sp_merkle_build_dev(uint64_t* levels, unsigned height, uint8_t* status, void* stream);
/* n_trees independent trees (any count) of the same height in lockstep: one launch pair per level
 * for all of them.  Leaves of tree t at felts [t 2^height, (t+1) 2^height); the buffer is level-major
 * with n_trees (2^(height+1) - 1) felts and ends with the n_trees roots. */
int sp_merkle_forest_dev(uint64_t* levels, size_t n_trees, unsigned height, uint8_t* status,
                         void* stream);
/* Sparse multi-update: root of the tree of the given height (<= 64) that holds new_leaves[i] at
 * keys[i] (strictly increasing) and `empty_leaf` everywhere else - the induced-subtree walk of
 * starkware/python/merkle_tree.py:4-26. */
int sp_merkle_sparse_root(const uint64_t* keys, const uint64_t* leaves, size_t n, unsigned height,
                          const uint64_t* empty_leaf, uint64_t* root, uint8_t* status);
/* Persistent sparse tree: merkle_multi_update{hash_ptr=pedersen_ptr} on a tree that already holds
 * state (services/perpetual/cairo/state/state.cairo:155-173; untouched siblings come from the previous
 * state, the role of `merkle_facts`, main.cairo:61-64).  The handle keeps, per level, the nodes that
 * differ from the empty-subtree root (an open-addressing table in HBM); sp_tree_update writes leaves[i] at keys[i]
 * (strictly increasing, < 2^height, height <= 64) in one call - one gathered launch per level - and
 * returns the root before and after.  status != 0 (SP_HASH_*) leaves the tree unchanged. */
int sp_tree_create(unsigned height, const uint64_t* empty_leaf, int* tree);
/* The same on context `context` of sp_init_devices (0 = the primary, what sp_tree_create uses): the tree's table,
 * stream and work buffer live on that device; every sp_tree_* call on the handle runs there. */
int sp_tree_create_on(int context, unsigned height, const uint64_t* empty_leaf, int* tree);
int sp_tree_update(int tree, const uint64_t* keys, const uint64_t* leaves, size_t n, uint64_t* old_root,
                   uint64_t* new_root, uint8_t* status);
int sp_tree_get(int tree, const uint64_t* keys, size_t n, uint64_t* leaves);
int sp_tree_root(int tree, uint64_t* root);
/* Witness export.  The Cairo program takes program_input['merkle_facts'] (services/perpetual/cairo/main.cairo:39-40,
 * 61-64): a dictionary node hash -> (left child, right child) that the two merkle_multi_update calls of
 * state/state.cairo:155-173 walk from the previous root and from the new root, along the subtree induced by the touched
 * leaves (starkware/python/merkle_tree.py:4-26).  The tree stores its nodes by position, so these calls read them back
 * by position: call sp_tree_witness with the batch's squashed keys before the update and again after it, and the union
 * of {node: (left, right)} over both results is the batch's merkle_facts for that tree.  Nothing is hashed. */
/* Number of witness records for `keys` in a tree of `height`: sum over levels 1..height of the number of distinct
 * keys[i] >> level.  Pure host arithmetic on the keys: callable before sp_init.  keys strictly increasing and
 * < 2^height, 1 <= height <= 64, else SP_ERR_BAD_ARGUMENT.  n == 0 gives 0. */
int sp_tree_witness_size(unsigned height, const uint64_t* keys, size_t n, size_t* n_records);
/* The merkle_facts of the subtree induced by `keys` in the tree AS IT STANDS (between updates).  One record per inner
 * node of the induced subtree, ordered by level (1 = parents of leaves ... height = the root), ascending index inside a
 * level:
 *   level[u], index[u]   position of the node
 *   node[u]              its value; left[u] / right[u]: the values at (level-1, 2 index) and (level-1, 2 index + 1)
 * A position the tree has never written reads as the empty-subtree root of its level.  *n_records always receives the
 * count.  capacity < count: SP_ERR_BAD_ARGUMENT, nothing else written.  Host pointers, synchronous.
 * SP_ERR_BAD_ARGUMENT with no output written at all: keys not strictly increasing, a key out of range for the tree's
 * height, an unknown or destroyed handle.
 * The call holds the tree's mutex from start to end, like sp_tree_get, so a witness always describes a batch boundary:
 * never a half-committed update.  One thread per record makes three table probes (the node and its two children); a
 * tree that has never been updated answers from the host's empty-subtree roots without a launch.
 * Size: a record is 105 bytes (1 + 8 + 3 x 32).  4096 keys on a height-64 tree give about 2 x 10^5 records, about 23 MB
 * back over PCIe: that copy, not the kernel, dominates the call (results up to 4 MiB go through the tree's page-locked
 * staging buffer, larger ones are copied directly, as an update's inputs are).  Measured (tools/quick_tree_witness.py,
 * profiles/tree_witness.txt): 0.54 ms per call, of which upload and kernels 0.09 ms, beside 1.46 ms for sp_tree_update
 * of the same keys; sp_tree_prove of the 4096 keys 0.23 ms. */
int sp_tree_witness(int tree, const uint64_t* keys, size_t n, size_t capacity, uint8_t* level, uint64_t* index,
                    uint64_t* node, uint64_t* left, uint64_t* right, size_t* n_records);
/* Inclusion proofs: leaves[i] = the leaf at keys[i] (as sp_tree_get: any order, repeats allowed) and
 * siblings[(i*height + l)] = the value at (l, (keys[i] >> l) ^ 1), l = 0..height-1 (felts: 4 words each).  Folding
 * leaves[i] with its siblings, H(left, right) level by level with bit l of keys[i] choosing the side, gives
 * sp_tree_root.  A key out of range or an unknown handle: SP_ERR_BAD_ARGUMENT, nothing written.  Same locking and
 * copy-back as sp_tree_witness; n x height (key, level) pairs must stay below 2^31. */
int sp_tree_prove(int tree, const uint64_t* keys, size_t n, uint64_t* leaves, uint64_t* siblings);
/* Ordered range scan: WHICH keys the tree holds.  Writes the first min(capacity, SP_TREE_SCAN_MAX, count) keys k with
 * lo <= k <= hi (both bounds inclusive, so 2^64 - 1 is reachable), ascending, whose leaf differs from the tree's empty
 * leaf; leaves receives the matching leaves (*n felts), *n the number written.  *more = 1 if and only if at least one
 * further such key exists in the range: resume with lo = keys[*n - 1] + 1.  A leaf that was written with the empty
 * leaf's value - never written, or set back - is not reported.  Host pointers, synchronous; locking and device
 * selection as sp_tree_get, so a page always describes a batch boundary.
 * The device walks down from the root, one step per level: the frontier of level l is the ascending list of nodes
 * whose key interval meets [lo, hi] and whose value differs from the empty-subtree root of level l; the frontier of
 * level 0 is the answer.  (1) Pruning compares VALUES, not presence: a leaf set back to the empty leaf leaves its path
 * in the table with empty-root values, and only a node that differs from its level's empty root has a live leaf below
 * it.  (2) Hence a frontier may be cut at any level - above level 0 to its first capacity + 2 nodes, since only the
 * first and the last node of a frontier can stick out of [lo, hi] and hold no leaf IN RANGE, so the first `capacity`
 * leaves lie below what is kept - and a cut at any level means `more`.  (3) No node interval is computed with a shift by
 * 64: the root's interval is "everything" and is never tested.
 * SP_ERR_BAD_ARGUMENT, with nothing written: lo > hi, hi >= 2^height when height < 64, capacity == 0, a null pointer,
 * an unknown or destroyed handle.  A tree that has never been updated, or whose root is the empty root, answers
 * *n = 0, *more = 0 without a launch.
 * Cost: proportional to height x *n table probes (one launch per level once the frontier is wider than one
 * workgroup, one launch for the narrow top; a page of up to 1022 keys is one launch), never to the size of the table;
 * one copy back (count, more, keys, leaves) through the tree's page-locked buffer for a page up to 4 MiB, above that
 * the count first and then exactly *n keys and leaves.  Measured numbers: DESIGN.md 4.8, tools/quick_tree_scan.py,
 * profiles/tree_scan.txt. */
/* capacity above SP_TREE_SCAN_MAX is treated as SP_TREE_SCAN_MAX: page with `more` */
#define SP_TREE_SCAN_MAX ((size_t)1 << 22)
int sp_tree_scan(int tree, uint64_t lo, uint64_t hi, size_t capacity,
                 uint64_t* keys, uint64_t* leaves, size_t* n, int* more);
/* The tree's node table as it stands: *entries = slots in use (nodes ever written, at any level: it never shrinks, a
 * leaf set back to the empty leaf keeps its path), *slots = the table's slot count (48 bytes each).  Read-only. */
int sp_tree_table_size(int tree, uint64_t* entries, uint64_t* slots);
/* A second handle holding the same tree: a checkpoint to roll back to, a fork to try a batch on, a base to diff against.
 * *clone receives a new handle on the context of `tree` with the same height, empty leaf and root; the node table (same
 * slot count) and its entry counter are copied device to device, nothing is hashed.  The clone has its own stream, work
 * buffer, staging buffer and mutex, made by its first call as a created tree's are.  The call holds the source's mutex
 * from start to end; the copies run on the source's stream, behind its last commit, and are finished when the call
 * returns.  Afterwards the two handles are independent: updating or destroying either leaves the other untouched.  A
 * tree that has never been updated has no table: its clone is a fresh tree of the same height and empty leaf, made
 * without device work.  The table is copied as it stands (a compacting copy is snapshot + restore).
 * SP_ERR_BAD_ARGUMENT, with nothing written: an unknown or destroyed handle, a null `clone`.  An allocation or copy
 * that fails returns SP_ERR_HIP: no handle is created and the source stays as it was.
 * Cost: the device-to-device copy of the table, 48 bytes per slot.  Measured (tools/quick_tree_diff.py,
 * profiles/tree_diff.txt): 1.67 ms for a height-64 tree of 2^18 keys (a 3.2 GB table), allocation
 * included, beside 32 ms for restoring its snapshot. */
int sp_tree_clone(int tree, int* clone);
/* Ordered diff: WHERE two trees differ.  Writes the first min(capacity, SP_TREE_DIFF_MAX, count) keys k with
 * lo <= k <= hi (both bounds inclusive, so 2^64 - 1 is reachable), ascending, whose leaf in tree_a differs from the
 * leaf in tree_b; leaves_a receives the leaf of A at each key and leaves_b the leaf of B (*n felts each), *n the number
 * written.  A key that a tree has never written, or has set back to the empty leaf, reads as the empty leaf.  *more = 1
 * if and only if at least one further differing key exists in the range: resume with lo = keys[*n - 1] + 1.  Host
 * pointers, synchronous.
 * The comparison is by VALUE: a position absent from a table reads as the empty-subtree root of its level, so a path
 * that A holds with empty-root values (a leaf written and set back) equals B's missing entry and is not reported.
 * The device walks down from the two roots, one step per level: the frontier of level l is the ascending list of nodes
 * whose key interval meets [lo, hi] and whose value in A differs from its value in B; the frontier of level 0 is the
 * answer.  (1) Both tables are consistent hash trees: equal leaves below a node give equal nodes, so a kept node has a
 * differing leaf below it, and equal nodes mean equal subtrees (up to a hash collision), so a pruned node has none.
 * (2) Hence a frontier may be cut at any level - above level 0 to its first capacity + 2 nodes, since only the first
 * and the last node of a frontier can stick out of [lo, hi] and hold no differing leaf IN RANGE - and a cut at any level
 * means `more`.  (3) No node interval is computed with a shift by 64: the root's interval is never tested.
 * SP_ERR_BAD_ARGUMENT, with nothing written: an unknown or destroyed handle, the same handle twice, trees of different
 * heights, of different empty leaves or on different contexts of sp_init_devices, lo > hi, hi >= 2^height when
 * height < 64, capacity == 0, a null pointer.  Equal roots - two trees never updated among them - answer *n = 0,
 * *more = 0 without a launch; ONE tree without a table is walked as a table in which every probe finds nothing.
 * Locking: both trees' mutexes from start to end, taken in ascending handle order whichever argument a tree is (as
 * sp_state_batch takes them: sp_tree_diff(a, b) beside sp_tree_diff(b, a) cannot block), so a page describes a batch
 * boundary of BOTH trees.  The work runs on the stream and in the work buffer of the lower handle, after a wait for the
 * other tree's stream.
 * Cost: proportional to height x *n, four table probes per node kept (two children in two tables, loaded together);
 * never to the size of either table.  Launches as sp_tree_scan's: one for the narrow top, which finishes a page of up to
 * 1022 keys alone, then one per level.  One copy back (count, more, keys, both runs of leaves) through the page-locked
 * buffer for a page up to 4 MiB, above that the count first and then exactly *n keys and two runs of *n leaves.
 * Measured (tools/quick_tree_diff.py, profiles/tree_diff.txt; height 64): a page of 4096 keys on two
 * trees that differ in all their 4096 keys 1.09 ms (device part 1.04 ms) beside 0.78 ms for sp_tree_scan of such a
 * page; 1.15 ms on two trees of 2^18 keys that differ in 4096, beside 9.6 ms for a snapshot of both and a compare on
 * the host; a page of 256 keys 0.59 ms. */
/* capacity above SP_TREE_DIFF_MAX is treated as SP_TREE_DIFF_MAX: page with `more` */
#define SP_TREE_DIFF_MAX SP_TREE_SCAN_MAX
int sp_tree_diff(int tree_a, int tree_b, uint64_t lo, uint64_t hi, size_t capacity,
                 uint64_t* keys, uint64_t* leaves_a, uint64_t* leaves_b, size_t* n, int* more);
/* Verifying inclusion proofs: Merkle paths folded on the device, all of a call in ONE launch (ped_fold_ragged_kernel)
 * that lasts as long as its longest path.  node = pedersen_hash(left, right) (signature.py:296-318); bit l of keys[i]
 * says whether the running node is the RIGHT child at level l (starkware/python/merkle_tree.py:4-26,
 * state/state.cairo:155-173): h <- H(sibling, h) if it is set, h <- H(h, sibling) if not, starting from h = leaves[i].
 *   off == NULL   every path has `height` siblings, sibling l of item i at siblings + 4 (i height + l): exactly the
 *                 layout sp_tree_prove writes, so its output is this call's input
 *   off != NULL   n + 1 HOST offsets in felts, off[0] = 0, non-decreasing; path i has off[i+1] - off[i] siblings
 *                 (0 .. 64) from siblings + 4 off[i]; `height` is ignored.  A path of no siblings folds to its leaf.
 *   keys          n HOST words in all three calls, like `off`; every bit at or above the path's length must be 0
 *   roots[i]      the folded root (n felts); status[i] (n bytes or NULL) = OR of the SP_HASH_* bytes of path i's
 *                 hashes: SP_HASH_OUT_OF_RANGE if the leaf (also of a path of no siblings) or a sibling is >= p
 *   expected      n_expected = 1 (one root for all paths) or n roots; verdict[i] = SP_PATH_TRUE only if status[i] is 0
 *                 and the folded root equals the expected one
 * SP_ERR_BAD_ARGUMENT, with nothing written: off[0] != 0, a decreasing offset, a path longer than 64, height > 64
 * while off is NULL, a key bit set at or above its path's length, n_expected outside {1, n}, more than 2^32 - 1
 * sibling felts.  n == 0 is SP_OK.
 * The _dev call takes leaves, siblings, roots and status on the device, enqueues and returns; it has copied `off`
 * and `keys` by then.  The host calls run on a host lane of the primary context (as sp_pedersen_chains_ragged);
 * sp_merkle_verify_paths compares on the device: only the n verdict bytes (and n status bytes when asked for) come
 * back over PCIe.  Batches above the largest launch class (8192 paths) go out as consecutive slices on the same
 * stream; without the quad kernels (or under STARKPERP_NO_PATH_FOLD=1) one gathered launch per level serves the call. */
#define SP_PATH_FALSE 0
#define SP_PATH_TRUE 1
int sp_merkle_fold_paths_dev(const uint64_t* leaves, const uint64_t* siblings, const uint32_t* off, unsigned height,
                             const uint64_t* keys, size_t n, uint64_t* roots, uint8_t* status, void* stream);
int sp_merkle_fold_paths(const uint64_t* leaves, const uint64_t* siblings, const uint32_t* off, unsigned height,
                         const uint64_t* keys, size_t n, uint64_t* roots, uint8_t* status);
int sp_merkle_verify_paths(const uint64_t* leaves, const uint64_t* siblings, const uint32_t* off, unsigned height,
                           const uint64_t* keys, size_t n, const uint64_t* expected, size_t n_expected,
                           uint8_t* verdict, uint8_t* status);
/* Verifying a multi-update from its witnesses: the statement of merkle_multi_update(prev_leaves, new_leaves, height,
 * prev_root, new_root) (state/state.cairo:155-173, the walk of starkware/python/merkle_tree.py:4-26 through
 * program_input['merkle_facts'], main.cairo:39-40, 61-64) checked against the records sp_tree_witness exports, without a
 * tree handle.  A record carries its node and both children, so no check waits for another: every record is hashed
 * once, all of them in ONE bulk launch sequence, and the rest is comparisons of felts (witness_check_kernel).
 *   keys          n HOST words, strictly increasing, < 2^height, 1 <= height <= 64 (in both calls, like the two roots)
 *   prev_leaves, new_leaves   n felts each: the leaf at keys[j] before and after the update
 *   n_records     must equal sp_tree_witness_size(height, keys, n) = R
 *   node, left, right   2 R felts each: the R records of the witness taken BEFORE the update, then the R records taken
 *                 AFTER it, both in sp_tree_witness's order (level 1 .. height, ascending index inside a level): two
 *                 sp_tree_witness outputs, one behind the other.  The POSITION of a record is never taken from the
 *                 caller: it follows from the keys alone, so a witness cannot claim one.
 *   status        2 R bytes (before half, then after half) or NULL; byte u is the OR of
 *                   SP_HASH_OUT_OF_RANGE, SP_HASH_UNHASHABLE   from hashing left[u], right[u] (a felt >= p is no bad
 *                                                 argument: it is SP_HASH_OUT_OF_RANGE on its record)
 *                   SP_WITNESS_HASH_MISMATCH      the status of the hash is 0 and H(left[u], right[u]) != node[u]
 *                   SP_WITNESS_LINK_MISMATCH      a child that lies on a key's path is not the node of the record at
 *                                                 (level - 1, 2 index + c) of the same half; at level 1 it is compared
 *                                                 with prev_leaves[j] / new_leaves[j] of that key
 *                   SP_WITNESS_SIBLING_CHANGED    a child on NO key's path differs between the before and the after
 *                                                 record of this position (set on both halves): the untouched side of
 *                                                 the tree must be the same node in the old and in the new tree
 *                   SP_WITNESS_ROOT_MISMATCH      last record of a half only: its node is not prev_root / new_root
 *   *verdict      SP_PATH_TRUE iff every one of the 2 R status bytes is 0, reduced on the device (it is preset and
 *                 cleared by one atomic per wave on the aligned 32-bit word that holds the byte)
 * n == 0: SP_OK, *verdict = (prev_root == new_root); n_records must be 0 and nothing else is read.
 * SP_ERR_BAD_ARGUMENT, with nothing written: keys not strictly increasing or out of range, a height outside 1 .. 64,
 * n_records != R, 2 R >= 2^31, a null pointer (status excepted).
 * The host call runs on a host lane like the other stateless host-pointer batches: it holds the library lock only to
 * enqueue, stages its inputs through page-locked memory up to 4 MiB and copies directly above that, and brings back
 * one byte (plus the 2 R status bytes when asked for).  The _dev call takes the felt arrays, status and verdict on the
 * device, keys and the two roots on the host; it enqueues on `stream` and returns once it has consumed keys and roots.
 * Cost: DESIGN.md 4.7, tools/quick_verify_update.py, profiles/verify_update.txt. */
#define SP_WITNESS_HASH_MISMATCH 0x04
#define SP_WITNESS_LINK_MISMATCH 0x08
#define SP_WITNESS_SIBLING_CHANGED 0x20
#define SP_WITNESS_ROOT_MISMATCH 0x40
int sp_merkle_verify_update_dev(unsigned height, const uint64_t* keys, size_t n, const uint64_t* prev_leaves,
                                const uint64_t* new_leaves, const uint64_t* prev_root, const uint64_t* new_root,
                                const uint64_t* node, const uint64_t* left, const uint64_t* right, size_t n_records,
                                uint8_t* verdict, uint8_t* status, void* stream);
int sp_merkle_verify_update(unsigned height, const uint64_t* keys, size_t n, const uint64_t* prev_leaves,
                            const uint64_t* new_leaves, const uint64_t* prev_root, const uint64_t* new_root,
                            const uint64_t* node, const uint64_t* left, const uint64_t* right, size_t n_records,
                            uint8_t* verdict, uint8_t* status);
/* Threading of the sp_tree_* calls (sp_tree_update, sp_tree_get, sp_tree_root, sp_tree_witness, sp_tree_prove,
 * sp_tree_scan, sp_tree_clone, sp_tree_diff, sp_tree_table_size, sp_tree_destroy): a tree has its own HIP stream, work buffer and mutex.  An operation holds
 * the tree's mutex from start to end and the library lock only while it enqueues; the device work of an update
 * (the level launches) runs without the library lock, so other trees and the stateless batches go on meanwhile. */
/* BASELINE.json configs[2] in one call (services/perpetual/cairo/order/limit_order.cairo:24-52, order.cairo:23-31,
 * :122-124): message-hash chains of n orders (words: depth x n felts, word-major; z_out receives the hashes) ->
 * verification of (z, r, s, key) through the key tables (verdicts as sp_ecdsa_verify_batch - a z of 2^251 or more is
 * SP_VERIFY_ASSERT_MSG and nothing is committed, constants.cairo:57 SIGNED_MESSAGE_BOUND; qy == NULL:
 * x-only keys) -> order id = bits [id_shift, id_shift + 64) of z (187 for the 251-bit message: the top 64 bits) ->
 * update of the orders tree `tree` with leaves[i] at order id i.  Verification and tree hashing overlap on the
 * device; the new nodes are committed only when every signature verified, otherwise *tree_status =
 * SP_TREE_NOT_COMMITTED and new_root = old_root.  Two orders with one id: SP_ERR_BAD_ARGUMENT.
 * Pinned by tests/test_gpu_order_batch.py:
 *   n == 0            SP_OK on a known tree: nothing is verified or written, *tree_status = 0, new_root = old_root
 *                     (an unknown handle is SP_ERR_BAD_ARGUMENT also then).
 *   tree_status       may be NULL; the outcome then shows as new_root == old_root.  z_out, verdicts, old_root and
 *                     new_root are required.
 *   a leaf >= p       *tree_status = SP_HASH_OUT_OF_RANGE (the byte of the tree's level hashing), nothing is
 *                     committed, the verdicts are those of the signatures.  The hash byte wins over
 *                     SP_TREE_NOT_COMMITTED: with a bad signature in the same batch the status is still the hash byte
 *                     (the tree is refused before the verifier's answer is asked for).
 *   a word >= p       at depth >= 2: *tree_status = the chains' SP_HASH_* byte, every verdict is 0, z_out is
 *                     unspecified, new_root = old_root.  At depth 1 nothing is hashed: the word IS the message hash,
 *                     and a word of 2^251 or more (>= p included) is SP_VERIFY_ASSERT_MSG as above.
 *   order ids         must be below 2^height of the tree, else SP_ERR_BAD_ARGUMENT with the tree unchanged (like
 *                     equal ids; z_out is written, the verdicts are unspecified).  id_shift <= 192, depth >= 1.
 *   a z >= 2^251      the batch ends after the verification: ids are not formed, so neither equal ids nor a leaf >= p
 *                     is reported beside it.
 * Host side: the verification runs on a thread of the call's own (spawned as soon as the message hashes are back,
 * parked until the tree update - the critical path - has enqueued its levels; joined before the call returns);
 * 4096 orders on a tree that holds state: 1.75 - 1.85 ms median, p90 within 7 %, against 1.51 ms of dependent
 * hashing (3 chain links + 64 tree levels; DESIGN.md 4.2, profiles/r06_c3_timeline.txt).  A tree's slot table that
 * must grow is sized for four times the need and grows without a device-wide wait; STARKPERP_TIMELINE=1 prints
 * the host-side marks of every call to stderr. */
int sp_order_batch(const uint64_t* words, size_t depth, size_t n, const uint64_t* r, const uint64_t* s,
                   const uint64_t* qx, const uint64_t* qy, int tree, const uint64_t* leaves, unsigned id_shift,
                   uint64_t* z_out, uint8_t* verdicts, uint64_t* old_root, uint64_t* new_root, uint8_t* tree_status);
/* The whole state update of a batch in one call: shared_state_apply_state_updates (services/perpetual/cairo/state/
 * state.cairo:135-186) - previous and new leaf of every touched position (position/hash.cairo:76-131), merkle_multi_update
 * of the positions tree (:155-161) and of the orders tree (:167-173) - all or nothing across BOTH trees.
 *   pos_keys, ord_keys   strictly increasing, below 2^height of their tree, squashed by the caller (state.cairo:67-96)
 *   prev_words/prev_off  previous leaf of position i = the left-fold chain over prev_words[4 prev_off[i] .. 4 prev_off[i+1])
 *                        (the convention of sp_pedersen_chains_ragged: n_pos + 1 offsets in felts, prev_off[0] = 0, every
 *                        chain at least one word)
 *   new_words/new_off    the new leaf likewise; a chain of length zero (new_off[i+1] == new_off[i]) says that the position
 *                        is unchanged: it is hashed once and its new leaf is its previous leaf
 *   ord_prev, ord_new    n_ord felts each: the orders-tree leaves before and after
 * Every previous leaf is compared ON THE DEVICE with what its tree holds at that key (the empty leaf for a key the tree
 * has never seen), every new node of both trees is hashed - the positions tree on its stream, the orders tree on its
 * own, side by side - and both tables are written only if everything checked out.  Otherwise neither is written, both
 * *_new_root equal their *_old_root and the call still returns SP_OK.
 *   *batch_status   0: committed; otherwise SP_TREE_NOT_COMMITTED OR-ed with every item status byte and with the
 *                   SP_HASH_* flags of the two trees' level hashing
 *   pos_status[i]   (n_pos bytes or NULL) OR of the SP_HASH_* bytes of item i's two chains; SP_STATE_PREV_MISMATCH is
 *                   added if, and only if, the previous chain's own status is 0 and its hash is not the tree's leaf
 *   ord_status[i]   (n_ord bytes or NULL) SP_HASH_OUT_OF_RANGE if ord_new[i] >= p; SP_STATE_PREV_MISMATCH if ord_prev[i]
 *                   is not the tree's leaf (a value >= p never is)
 * SP_ERR_BAD_ARGUMENT, with no output written: keys not strictly increasing or out of range for the tree's height;
 * off[0] != 0, a decreasing offset or a previous chain of length zero; an unknown handle; the same handle twice; two
 * trees on different contexts of sp_init_devices (not supported: both trees of one state live on one device).
 * n_pos == 0 and / or n_ord == 0 are legal: a tree with nothing to write reports old == new and still takes part in
 * the all-or-nothing decision.
 * No hash crosses PCIe: the call uploads the words, one ragged launch sequence hashes previous and new chains into the
 * positions tree's work buffer, a leaf kernel per tree looks the current leaves up, compares, writes the status bytes
 * and places the new leaves where the update's level 0 is read from.  Host side: the call holds both trees' mutexes
 * from start to end (always taken in ascending handle order, so callers that name the same two trees in opposite
 * roles cannot block each other) and the library lock only while it enqueues; it takes no host lane and starts no
 * thread.  STARKPERP_TIMELINE=1 prints its host-side marks like sp_order_batch's.  Timing: tools/quick_state_batch.py. */
#define SP_STATE_PREV_MISMATCH 0x10 /* per item: the previous value given is not what the tree holds */
int sp_state_batch(int positions_tree, int orders_tree, const uint64_t* pos_keys, size_t n_pos,
                   const uint64_t* prev_words, const uint32_t* prev_off, const uint64_t* new_words,
                   const uint32_t* new_off, const uint64_t* ord_keys, const uint64_t* ord_prev,
                   const uint64_t* ord_new, size_t n_ord, uint64_t* pos_old_root, uint64_t* pos_new_root,
                   uint64_t* ord_old_root, uint64_t* ord_new_root, uint8_t* pos_status, uint8_t* ord_status,
                   uint8_t* batch_status);
int sp_tree_destroy(int tree);

/* ---- Stark-curve ECDSA ------------------------------------------------------------------------ */
/* verify(msg_hash, r, s, public_key) signature.py:217-260.  qy == NULL: public keys are x-only
 * (both y candidates are tried, signature.py:229-238). */
int sp_ecdsa_verify_batch(const uint64_t* z, const uint64_t* r, const uint64_t* s,
                          const uint64_t* qx, const uint64_t* qy, uint8_t* result, size_t n);
int sp_ecdsa_verify_batch_dev(const uint64_t* z, const uint64_t* r, const uint64_t* s,
                              const uint64_t* qx, const uint64_t* qy, uint8_t* result, size_t n,
                              void* stream);
/* Key tables - the same verify() for public keys that are seen again (an exchange's accounts):
 * a registered key owns four 128-entry signed comb tables (32 KiB, on Q, 2^8 Q, 2^16 Q, 2^24 Q) in HBM that
 * replace the 252 doublings + 63 additions of the per-signature ladder by 7 doublings + 31 mixed additions.  Results are
 * identical to sp_ecdsa_verify_batch for every input (same pre-asserts, same False cases).
 *   sp_ecdsa_register_keys  host pointers; qy == NULL registers x-only keys; equal keys share a
 *                           slot; slots[i] receives the slot of key i; keys that are not on the curve own
 *                           no table - they share two sentinel slots (their verifications return False /
 *                           SP_VERIFY_ASSERT_CURVE as before) and are remembered on the host, so an
 *                           untrusted key stream cannot fill the cache;
 *                           SP_ERR_CACHE_FULL when no slot is free (ceiling: 2^17 keys = 4 GiB, or
 *                           STARKPERP_KEY_CACHE_SLOTS; the tables are allocated lazily, 128 MiB first, doubling),
 *                           in which case nothing is registered.
 *   sp_ecdsa_verify_keyed_dev  device pointers; slots[i] names the key of signature i.
 *   sp_ecdsa_verify_batch_keyed  host pointers: registers what is new, then verifies.
 * sp_ecdsa_verify_batch itself switches to the tables when at most 40 % of a batch's signatures bring
 * a key the library has never met (not registered, not seen in an earlier call, not repeated inside the
 * batch) - so a caller verifying one signature at a time reaches the tables on the second sighting of
 * a key.  That default (SP_VERIFY_POLICY_AUTO) makes sp_ecdsa_verify_batch remember keys between calls and
 * allocate the key cache on first use; sp_ecdsa_set_verify_policy chooses otherwise for the whole process:
 *   SP_VERIFY_POLICY_LADDER  sp_ecdsa_verify_batch never looks at, fills or allocates the key cache - the
 *                            stateless-after-init function of the reference; tables only through the
 *                            explicit calls above; selecting it also forgets the keys seen so far;
 *   SP_VERIFY_POLICY_KEYED   always through the tables (the ladder only for a batch with more keys than the cache holds).
 * When the policy path (AUTO / KEYED) finds the cache full it EVICTS: a new slot generation, as after
 * sp_ecdsa_key_cache_reset - handles obtained from sp_ecdsa_register_keys before that answer SP_VERIFY_STALE_SLOT.
 * sp_ecdsa_verify_batch_keyed runs on a host lane: the library lock is held to register new keys and to enqueue,
 * not while the caller waits for the device.
 * STARKPERP_VERIFY_KEYED=0 / 1 in the environment selects LADDER / KEYED as the initial policy.  The verdicts do
 * not depend on the policy. */
#define SP_VERIFY_POLICY_AUTO 0
#define SP_VERIFY_POLICY_LADDER 1
#define SP_VERIFY_POLICY_KEYED 2
int sp_ecdsa_set_verify_policy(int policy);
int sp_ecdsa_get_verify_policy(void);
int sp_ecdsa_register_keys(const uint64_t* qx, const uint64_t* qy, size_t n, uint32_t* slots);
int sp_ecdsa_verify_keyed_dev(const uint64_t* z, const uint64_t* r, const uint64_t* s,
                              const uint32_t* slots, uint8_t* result, size_t n, void* stream);
int sp_ecdsa_verify_batch_keyed(const uint64_t* z, const uint64_t* r, const uint64_t* s,
                                const uint64_t* qx, const uint64_t* qy, uint8_t* result, size_t n);
int sp_ecdsa_key_cache_info(size_t* capacity, size_t* used);
/* Empties the cache after waiting for the device and starts a new slot generation.  A slot handle is
 * (generation << 24) | index; handles from before the reset are answered with SP_VERIFY_STALE_SLOT by
 * sp_ecdsa_verify_keyed_dev (never with another key's verdict): callers register their keys again. */
int sp_ecdsa_key_cache_reset(void);
/* ---- signing: what the batch signer is for, and its threat model ------------------------------------------
 * The batch signer exists to MAKE order batches (BASELINE configs[2]: 4096 signed limit orders) - test vectors,
 * load generators, a market maker that signs its own quotes on its own device.  It is NOT a hardened signing
 * service for keys of third parties on a device shared with untrusted tenants:
 *   data-independent   the RFC 6979 nonce derivation (HMAC-SHA256: fixed schedule, no secret-dependent branch or
 *                      address), both inversions that involve secrets (k^-1 and the (z + r d) denominator: fixed
 *                      length Bernstein-Yang divsteps, 21 x 29 branch-free steps, identical for every lane,
 *                      fp29.hpp), all field / scalar multiplications (no secret-dependent branches);
 *   NOT independent    k*G and d*G are sums of EC_GEN table entries gathered from HBM at addresses that are windows
 *                      of the secret scalar (12 random 64-byte reads per nonce at the default 21-bit windows): an
 *                      observer of the memory system of the SAME device (another process time-slicing the GPU, a
 *                      co-tenant with cache / HBM-channel contention counters) can learn bits of k; the nonce
 *                      pipeline's compaction makes the NUMBER of rejected candidates of an item visible in timing
 *                      (it depends on k's HMAC chain, not on d); the exceptional-case branches of the attempt
 *                      (r = 0, out-of-range w: 2^-55 events) are data dependent;
 *   at rest            nonces and HMAC states of the compacted pipeline are scrubbed on the stream behind their
 *                      last reader, staged private keys and nonces of the host-pointer calls likewise, and their
 *                      copy in the lane's page-locked block is zeroed before the call returns; r, s and the public
 *                      key are public.  Buffers the CALLER owns (d in the _dev calls) are the caller's to scrub.
 * The reference is no different in kind: signature.py:137-173 signs with Python big integers, a recursive
 * double-and-add ec_mult whose branches follow the bits of k (math_utils.py:91-100) and sympy's variable-time
 * igcdex - it is not constant-time either.
 * STARKPERP_SIGN_MASKED=1 (read by sp_init) removes the address dependence: the signers and sp_public_key_batch then
 * walk a second EC_GEN table of 63 unsigned 4-bit windows (63 KiB), reading ALL 16 entries of every window - the
 * same addresses on every lane whatever the scalar is - and keeping one by a mask; 62 mixed additions for every k.
 * Checked on the ISA, not only at source level: tests/test_masked_walk_isa.py compiles the walk (csrc/masked_walk.hpp)
 * for gfx950 and asserts that every table entry is fetched by wave-uniform scalar loads, that EXEC is never written
 * and that the only branch is the uniform loop counter's; inside the signer kernels the mask passes an opaque-value
 * barrier so that the compiler cannot re-derive a branch from it.
 * Same keys and signatures bit for bit (tests/test_gpu_ecdsa.py::test_masked_signer_...); 2^16 signatures 0.86 ->
 * 1.27 ms (7.7 -> 5.2 x 10^7 /s), d * G four times slower (profiles/r05_masked_signer.txt).  What stays data
 * dependent under the mask: the number of rejected RFC 6979 candidates (timing of the nonce phase) and the 2^-55
 * exceptional branches.  A deployment that must sign third-party keys on a shared device should still keep its HSM
 * / constant-time CPU signer and use this library for hashing and verification (which handle public data only).
 *
 * One signing attempt per item with caller-supplied nonce k (host RFC 6979, signature.py:117-134):
 * the body of the loop at signature.py:146-173. */
int sp_ecdsa_sign_batch(const uint64_t* z, const uint64_t* d, const uint64_t* k, uint64_t* r,
                        uint64_t* s, uint8_t* status, size_t n);
/* The whole of sign(msg_hash, priv_key, seed) signature.py:137-173 on the device: the RFC 6979 nonce
 * (HMAC-SHA256, python-ecdsa conventions, signature.py:117-134), the attempt, and the reference's
 * retry with the next seed.  seeds: one uint64 per item (0 = no seed; NULL = none for every item).
 * status SP_SIGN_RETRY after 8 rejected nonces in a row (a 2^-55 event each) leaves the item to the
 * caller. */
int sp_ecdsa_sign_rfc6979_batch(const uint64_t* z, const uint64_t* d, const uint64_t* seeds, uint64_t* r,
                                uint64_t* s, uint8_t* status, size_t n);
/* The two signing calls on DEVICE pointers (signature.py:137-173 per item, as above): enqueued on `stream`,
 * nothing staged and nothing waited for - the batch signer of a device-resident pipeline (message hashes left
 * in HBM by sp_pedersen_chains_dev are signed where they lie).  status is required; r / s of an item whose
 * status is not SP_SIGN_OK are left as they were.  seeds may be NULL (no seed for any item).
 * Launches and scratch: sp_ecdsa_sign_batch_dev is ONE launch with no shared state.
 * sp_ecdsa_sign_rfc6979_batch_dev is one launch below 4096 items; from 4096 items on the nonce phase runs as
 * rounds over the compacted list of rejected candidates - 15 launches and one scrubbing memset per chunk of at
 * most 2^20 items (STARKPERP_SIGN_CHUNK) - on 232 bytes of per-stream scratch per item of a chunk (at most
 * 290 MiB per stream).  The first such call on a stream allocates the scratch (hipMalloc: a device-wide
 * synchronisation, not capturable into a hipGraph): warm the stream up first, or set STARKPERP_SIGN_COMPACT_MIN=0
 * to keep the one-launch signer at every size (same signatures, 2.0 instead of 2.9 x 10^8 /s at 2^20 items).  If
 * the scratch cannot be allocated the call falls back to the one-launch signer instead of failing. */
int sp_ecdsa_sign_batch_dev(const uint64_t* z, const uint64_t* d, const uint64_t* k, uint64_t* r, uint64_t* s,
                            uint8_t* status, size_t n, void* stream);
int sp_ecdsa_sign_rfc6979_batch_dev(const uint64_t* z, const uint64_t* d, const uint64_t* seeds, uint64_t* r,
                                    uint64_t* s, uint8_t* status, size_t n, void* stream);
/* private_key_to_ec_point_on_stark_curve signature.py:104-106: (qx, qy) = d * EC_GEN.
 * status: 0 ok, 2 when d is not in (0, EC_ORDER). */
int sp_public_key_batch(const uint64_t* d, uint64_t* qx, uint64_t* qy, uint8_t* status, size_t n);
/* The same on device pointers (qy, status may be NULL; outputs of a rejected item are left as they were). */
int sp_public_key_batch_dev(const uint64_t* d, uint64_t* qx, uint64_t* qy, uint8_t* status, size_t n, void* stream);

/* ---- square roots mod p, x-only Stark keys ---------------------------------------------------------- */
/* per-item status of sp_felt_sqrt_batch* and sp_stark_key_y_batch* */
#define SP_SQRT_OK 0
#define SP_SQRT_NON_RESIDUE 1   /* no root: get_y_coordinate raises InvalidPublicKeyError, is_valid_stark_key is False */
#define SP_SQRT_OUT_OF_RANGE 2  /* the input is not in [0, p) */
/* sqrt_mod(a, FIELD_PRIME) math_utils.py:43-47 with is_quad_residue math_utils.py:36-40 as its status: root[i] is the
 * smaller of the two roots of a[i] when status[i] is SP_SQRT_OK (a = 0: root 0, OK, as sympy counts it) and is left as
 * it was otherwise.  status is required and written for every item, exactly.  root == NULL asks for the status bytes
 * alone (the Legendre symbol: no root is extracted).  n == 0 is legal.  a and root must not overlap (equal pointers:
 * SP_ERR_BAD_ARGUMENT; lanes past the end of the batch redo its last item).  A fixed number of field operations for
 * every in-range non-zero input, residue or not (2 338 against up to 18 528 squarings of Tonelli-Shanks for this prime,
 * whose 2-part has order 2^192): csrc/fp29.hpp fe_sqrt.  The first root call of a context builds and uploads its
 * 204 KiB of tables under the library lock (an allocation: not capturable into a hipGraph - call once before a
 * capture); sp_shutdown frees them; sp_table_bytes does not count them.  The host call runs on a host lane. */
int sp_felt_sqrt_batch(const uint64_t* a, uint64_t* root, uint8_t* status, size_t n);
/* The same on device pointers, on the device they live on: enqueued on `stream`, nothing waited for. */
int sp_felt_sqrt_batch_dev(const uint64_t* a, uint64_t* root, uint8_t* status, size_t n, void* stream);
/* get_y_coordinate signature.py:84-96: qy[i] = the smaller root of qx^3 + qx + beta, status SP_SQRT_NON_RESIDUE where
 * the reference raises InvalidPublicKeyError.  qy == NULL: is_valid_stark_key signature.py:204-214 alone, in the
 * status bytes.  qx is NOT reduced mod p (SP_SQRT_OUT_OF_RANGE); everything else as sp_felt_sqrt_batch. */
int sp_stark_key_y_batch(const uint64_t* qx, uint64_t* qy, uint8_t* status, size_t n);
int sp_stark_key_y_batch_dev(const uint64_t* qx, uint64_t* qy, uint8_t* status, size_t n, void* stream);

/* ---- point arithmetic on the Stark curve: k P, a EC_GEN + b P, P +- Q ---------------------------------- */
/* ec_mult / ec_add / ec_double of math_utils.py:59-100 on the Stark curve (alpha = 1, p = FIELD_PRIME), one item per
 * lane.  Points are affine, x and y in arrays of their own like qx / qy above; scalars are plain 256-bit integers.
 * per-item status, written for every item, exactly: */
#define SP_EC_OK 0
#define SP_EC_INFINITY 1      /* the result is the point at infinity, which has no affine form (the reference's ec_add /
                                 ec_double assert there) */
#define SP_EC_OUT_OF_RANGE 2  /* a coordinate is not in [0, p) or a scalar is not in [0, EC_ORDER); nothing is reduced */
#define SP_EC_NOT_ON_CURVE 3  /* an input point fails y^2 = x^3 + x + beta */
/* The checks run in that order - the range of every input of the item first, then the curve, then the arithmetic - and
 * every input point is checked even when its scalar is 0.  rx / ry of an item whose status is not SP_EC_OK are left as
 * they were.  ry == NULL asks for x alone; status and rx are required; n == 0 is legal.  An output array that overlaps
 * an input array is SP_ERR_BAD_ARGUMENT (lanes past the end of the batch redo its last item, so in-place would race).
 * A scalar of 0 is legal: k = 0 gives SP_EC_INFINITY, and in sp_ec_lincomb_batch a zero term drops out.  The result is
 * the right point or SP_EC_INFINITY for EVERY pair of operands: b P == a EC_GEN (the sum is a doubling), b P ==
 * -(a EC_GEN) (infinity), P == Q, P == -Q, and the two scalars (30 and EC_ORDER - 30) at which the verifier's ladder
 * would meet its own operand.
 *
 * What these calls are for, in the terms of the signer's section above: PUBLIC data, or the caller's own secrets on the
 * caller's own device.  k P and b P run the verifier's signed 4-bit window ladder, which reads its per-lane table of
 * the eight odd multiples of P at addresses that are digits of the scalar, and a EC_GEN gathers EC_GEN table entries
 * at addresses that are windows of a; the field inversions (two per ladder item) may be variable-time.  a EC_GEN
 * always walks the gathered EC_GEN table of the verifier: the masked table of STARKPERP_SIGN_MASKED=1 is bypassed
 * deliberately, since the ladder beside it is address-dependent anyway.
 * Scratch: the ladder's table is 8 x 36 limbs x 4 bytes = 1152 bytes per lane, per stream, grown by the first call on a
 * stream that needs more (hipMalloc: a device-wide synchronisation, not capturable into a hipGraph - call once at the
 * largest n before a capture) and freed by sp_shutdown.  sp_ec_add_batch needs none.  The host calls run on a host lane. */
/* R = k P */
int sp_ec_mult_batch(const uint64_t* k, const uint64_t* px, const uint64_t* py, uint64_t* rx, uint64_t* ry,
                     uint8_t* status, size_t n);
/* R = a EC_GEN + b P */
int sp_ec_lincomb_batch(const uint64_t* a, const uint64_t* b, const uint64_t* px, const uint64_t* py, uint64_t* rx,
                        uint64_t* ry, uint8_t* status, size_t n);
/* R = P + Q, or P - Q when subtract != 0 */
int sp_ec_add_batch(const uint64_t* px, const uint64_t* py, const uint64_t* qx, const uint64_t* qy, int subtract,
                    uint64_t* rx, uint64_t* ry, uint8_t* status, size_t n);
/* The same on device pointers, on the device they live on: enqueued on `stream`, nothing waited for. */
int sp_ec_mult_batch_dev(const uint64_t* k, const uint64_t* px, const uint64_t* py, uint64_t* rx, uint64_t* ry,
                         uint8_t* status, size_t n, void* stream);
int sp_ec_lincomb_batch_dev(const uint64_t* a, const uint64_t* b, const uint64_t* px, const uint64_t* py,
                            uint64_t* rx, uint64_t* ry, uint8_t* status, size_t n, void* stream);
int sp_ec_add_batch_dev(const uint64_t* px, const uint64_t* py, const uint64_t* qx, const uint64_t* qy, int subtract,
                        uint64_t* rx, uint64_t* ry, uint8_t* status, size_t n, void* stream);

/* ---- prover-side transforms over GF(p) (build-defined: the reference has no prover) -------------- */
/* Field and generator: pedersen_params.json:20-21 (FIELD_PRIME, FIELD_GEN = 3).  All pointers are
 * device pointers to plain felts unless named *_host.                                            */
/* Radix-2 NTT of 2^log_n felts, natural order in and out; inverse != 0 divides by n. */
int sp_ntt_dev(const uint64_t* in, uint64_t* out, unsigned log_n, int inverse, void* stream);
/* Coset low-degree extension of ncols columns (column c at in + c * 2^log_n felts) from <w_n> to
 * shift * <w_{n * 2^log_blowup}>, natural order; out holds ncols * 2^(log_n + log_blowup) felts.  Any log_blowup
 * with log_n + log_blowup <= 26 (SP_ERR_BAD_ARGUMENT above that); up to 11 the zero padding happens inside the first
 * pass, above it the padded columns are written out first. */
int sp_lde_dev(const uint64_t* in, uint64_t* out, unsigned ncols, unsigned log_n, unsigned log_blowup,
               const uint64_t* shift_host, void* stream);
/* Rules shared by the calls below.
 *   Empty calls: a witness generator (sp_pedersen_trace_dev, sp_ec_ladder_trace_dev, sp_ecdsa_trace_dev,
 *     sp_range_check_trace_dev, sp_rc16_trace_dev) given a count of 0 and sp_air_eval_shard_dev given n_points = 0
 *     return SP_OK: nothing is reserved, launched or written.  A fold shard of count = 0 returns SP_OK too.
 *   Composition calls (sp_air_eval_dev, _shard_dev, _blocks_dev, sp_air_eval_ec_ladder_dev, sp_air_eval_ecdsa_dev,
 *     sp_air_eval_range_check_dev, sp_air_eval_rc16_dev): log_n is the trace length and is at least the AIR's period
 *     - 9 .. 30 for the Pedersen-step AIR (all three of its calls; the shard calls take the GLOBAL log_n), 8 .. 30
 *     for the EC ladder, 10 .. 30 for ECDSA, 7 .. 30 for the range check, 3 .. 24 for rc16 - and the shift is
 *     neither 0 nor a felt with shift^n * w_4^k = 1 for some k (that is shift^(4n) = 1: 1, p - 1, any power of
 *     w_{4n}): x^n - 1 vanishes on such a coset and the column does not exist.  Either violation is
 *     SP_ERR_BAD_ARGUMENT before anything is launched; sp_last_error() names the call and says "log_n" or "shift".
 *   Folds (sp_fri_fold_dev, _shard_dev, _blocks_dev): a shift of 0 is SP_ERR_BAD_ARGUMENT (the fold divides by 2 x). */
/* Execution trace of the Pedersen-step AIR: 512 rows per hash, columns s, px, py, lambda
 * (cols = 4 columns of 512 * n_hashes felts).  Step relation: signature.py:305-317 with the chord
 * rule of math_utils.py:59-68. */
int sp_pedersen_trace_dev(const uint64_t* x, const uint64_t* y, size_t n_hashes, uint64_t* cols,
                          void* stream);
/* Composition column sum_k alpha_k C_k(x) / (x^n - 1) on the blowup-4 coset.  trace_lde: 4 columns of
 * 4 * 2^log_n felts; periodic_lde: 6 tables of 2048 felts; alphas_host: 11 felts.  9 <= log_n <= 30. */
int sp_air_eval_dev(const uint64_t* trace_lde, const uint64_t* periodic_lde, unsigned log_n,
                    const uint64_t* alphas_host, const uint64_t* shift_host, uint64_t* out, void* stream);
/* Row shard of the same column for one rank of a multi-GPU job (SURVEY 8(e) "AIR eval": LDE-row shards
 * with a halo of one trace row): n_points LDE points from global index row0 (a multiple of 4); the four
 * columns are col_stride felts apart and hold n_points + 4 rows, the last four received from the owner of
 * the following rows (the owner of the last rows receives rows 0 .. 3).  log_n is the global trace length.
 * SP_ERR_BAD_ARGUMENT: row0 not a multiple of 4, col_stride < n_points + 4, row0 + n_points > 4 * 2^log_n. */
int sp_air_eval_shard_dev(const uint64_t* trace_lde, size_t col_stride, size_t n_points, size_t row0,
                          const uint64_t* periodic_lde, unsigned log_n, const uint64_t* alphas_host,
                          const uint64_t* shift_host, uint64_t* out, void* stream);
/* EC-ladder AIR (one mimic_ec_mult_air instance = 256 rows, signature.py:176-190): witness columns
 * m, px, py, qx, qy, la, ld for n_ladders scalar multiplications m * (qx, qy) + SHIFT_POINT
 * (cols = 7 columns of 256 * n_ladders felts), and its composition column (12 constraints,
 * periodic_lde: 3 tables of 1024 felts). */
int sp_ec_ladder_trace_dev(const uint64_t* m, const uint64_t* qx, const uint64_t* qy, size_t n_ladders,
                           uint64_t* cols, void* stream);
int sp_air_eval_ec_ladder_dev(const uint64_t* trace_lde, const uint64_t* periodic_lde, unsigned log_n,
                              const uint64_t* alphas_host, const uint64_t* shift_host, uint64_t* out,
                              void* stream);
/* Range-check AIR (what the Cairo range-check builtin asserts for every amount, position id, nonce and
 * expiration of the exchange messages, e.g. signature_message_hashes.cairo:60-75 via assert_nn_le /
 * the 2^64, 2^32 bounds of perpetual_messages.py:226-236): 0 <= value < 2^128 by bit decomposition,
 * 128 rows of one column per value (col = 128 * n_values felts, v_i = value >> i), and its composition
 * column (2 constraints, periodic_lde: 2 tables of 512 felts).  A value >= 2^128 gives a trace whose
 * composition is not a polynomial: the proof fails at the verifier, nothing is rejected here. */
int sp_range_check_trace_dev(const uint64_t* values, size_t n_values, uint64_t* col, void* stream);
int sp_air_eval_range_check_dev(const uint64_t* trace_lde, const uint64_t* periodic_lde, unsigned log_n,
                                const uint64_t* alphas_host, const uint64_t* shift_host, uint64_t* out,
                                void* stream);
/* The range-check BUILTIN as an AIR segment (oracle/stark_ref.py "rc16"; what the Cairo program's
 * `range_check` builtin - services/perpetual/cairo/main.cairo:1, used at order/order.cairo:53-56 - asserts):
 * a value < 2^128 is eight 16-bit limbs, 8 rows of the columns a (limb), acc (running value) and s (the limb
 * column SORTED: neighbours differ by 0 or 1, first = rc_min, last = rc_max); after these are committed a
 * challenge z is drawn and the second-phase column p_i = prod_{j <= i} (z - a_j) / (z - s_j) proves that s is a
 * permutation of a.  sp_rc16_trace_dev writes a and acc (cols = 2 columns of 8 * n_values felts; the caller
 * sorts a into s); sp_rc16_product_dev writes p (n felts); sp_air_eval_rc16_dev the rc16 part of the
 * composition column (cols: a, acc, s of 4 * 2^log_n felts each; periodic_lde: 2 tables of 32 felts;
 * alphas_host: 8 felts) - transition, all-but-last-row and boundary constraints.  sp_felt_add_dev sums the
 * composition parts of the segments of a combined trace.
 * sp_rc16_product_dev PRECONDITION, not checked: z differs from every s_j.  The denominators z - s_j are inverted
 * in groups of 16 consecutive cells with one inversion per group; a z that equals some s_j zeroes that group's
 * product, so all 16 quotients of the group come out 0 and every p_i from the group's first cell to the end of the
 * column is 0 - with SP_OK.  z is a Fiat-Shamir challenge over the whole field and s_j < 2^16, so a prover never
 * meets this; a caller that picks z by hand must avoid the values of s. */
int sp_rc16_trace_dev(const uint64_t* values, size_t n_values, uint64_t* cols, void* stream);
int sp_rc16_product_dev(const uint64_t* a, const uint64_t* s, size_t n, const uint64_t* z_host, uint64_t* p,
                        void* stream);
int sp_air_eval_rc16_dev(const uint64_t* cols, const uint64_t* p, const uint64_t* periodic_lde, unsigned log_n,
                         const uint64_t* alphas_host, const uint64_t* shift_host, const uint64_t* z_host,
                         uint64_t rc_min, uint64_t rc_max, uint64_t* out, void* stream);
int sp_felt_add_dev(const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n, void* stream);
/* ECDSA-verification AIR (what verify() mimics, signature.py:217-260): three linked EC ladders per
 * signature - z G from MINUS_SHIFT_POINT, r Q and w B from SHIFT_POINT with B = zG + rQ (:252-254) - and
 * x(wB - SHIFT_POINT) == r (:255); 1024 rows of ten columns m, px, py, qx, qy, la, ld, cx, cy, cr per
 * signature (cols = 10 columns of 1024 * n_sigs felts).  w = s^-1 mod N is an input, as in the reference
 * (:220: verify computes it before mimicking the AIR).  Composition: 26 constraints, periodic_lde = 12
 * tables of 4096 felts. */
int sp_ecdsa_trace_dev(const uint64_t* z, const uint64_t* r, const uint64_t* w, const uint64_t* qx,
                       const uint64_t* qy, size_t n_sigs, uint64_t* cols, void* stream);
int sp_air_eval_ecdsa_dev(const uint64_t* trace_lde, const uint64_t* periodic_lde, unsigned log_n,
                          const uint64_t* alphas_host, const uint64_t* shift_host, uint64_t* out, void* stream);
/* One FRI fold of f on shift * <w_M> (M = 2^log_m) to g on shift^2 * <w_{M/2}>:
 * g(x^2) = (f(x) + f(-x)) / 2 + beta (f(x) - f(-x)) / (2 x). */
int sp_fri_fold_dev(const uint64_t* in, uint64_t* out, unsigned log_m, const uint64_t* beta_host,
                    const uint64_t* shift_host, void* stream);
/* Row shard of one fold: out[i] = fold(fa[i], fb[i]) for the global positions i0 .. i0 + count of a layer of
 * 2^log_m points; fa = f[i0 ..], fb = f[i0 + 2^(log_m - 1) ..] (the second array comes from the rank that
 * owns the upper half of the layer). */
int sp_fri_fold_shard_dev(const uint64_t* fa, const uint64_t* fb, uint64_t* out, unsigned log_m, size_t i0,
                          size_t count, const uint64_t* beta_host, const uint64_t* shift_host, void* stream);
/* Block-cyclic row shards (one job over the GPUs of a node, starkperp/sharded_prover.py; SURVEY 8(e) rows "AIR
 * eval" and "FRI"): the LDE rows / layer positions are cut into blocks of 2^log_block consecutive indices and
 * block b belongs to rank b mod world, local block t being global block t * world + rank.  The next-row reads
 * of the AIR stay inside a block plus a halo of one trace row, and both members (i, i + M/2) of every fold pair
 * live on the same rank while M/2 >= world * 2^log_block - no data moves between folds.
 *   sp_air_eval_blocks_dev   trace_lde: 4 columns col_stride felts apart, n_blocks blocks stored 2^log_block + 4
 *                            rows apart (block + halo); out: n_blocks * 2^log_block composition values.
 *   sp_fri_fold_blocks_dev   fa / fb: the rank's `count` positions of the lower / upper half of the layer. */
int sp_air_eval_blocks_dev(const uint64_t* trace_lde, size_t col_stride, size_t n_blocks, unsigned log_block,
                           unsigned world, unsigned rank, const uint64_t* periodic_lde, unsigned log_n,
                           const uint64_t* alphas_host, const uint64_t* shift_host, uint64_t* out, void* stream);
int sp_fri_fold_blocks_dev(const uint64_t* fa, const uint64_t* fb, uint64_t* out, unsigned log_m, size_t count,
                           unsigned log_block, unsigned world, unsigned rank, const uint64_t* beta_host,
                           const uint64_t* shift_host, void* stream);
/* The two halves of sp_lde_dev (blowup 1) as separate calls, so that the coset transforms of one column share a
 * single interpolation: evaluations on <w_n> -> coefficients in BIT-REVERSED order -> evaluations on
 * shift * <w_n> (natural order).  ncols columns 2^log_n felts apart.  The intermediate array holds n times each
 * coefficient (the 1/n is applied by sp_coset_eval_dev): it is meant for sp_coset_eval_dev alone. */
int sp_interpolate_dev(const uint64_t* in, uint64_t* coef, unsigned ncols, unsigned log_n, void* stream);
int sp_coset_eval_dev(const uint64_t* coef, uint64_t* out, unsigned ncols, unsigned log_n,
                      const uint64_t* shift_host, void* stream);
/* Commit (build-defined): Pedersen-Merkle tree over the rows of a column-major table of
 * n_rows (a power of two) x n_cols felts; leaf = left-fold chain of the row's felts (one column: the
 * felt itself).  levels receives 2 n_rows - 1 felts, leaves first, root last.  Passing a status
 * pointer makes the call wait for the stream. */
int sp_commit_rows_dev(const uint64_t* cols, size_t n_rows, size_t n_cols, uint64_t* levels, uint8_t* status,
                       void* stream);
/* Opening committed tables: the prover's half of the query phase.  ONE launch (commit_open_kernel) reads every
 * opened row and every Merkle sibling of a call out of tables that sp_commit_rows_dev committed, and writes the
 * layout that sp_merkle_fold_paths / sp_merkle_verify_paths take in their off != NULL form - as sp_tree_prove does
 * for the persistent trees.
 *   table t       cols[t]: DEVICE pointer to n_rows[t] x n_cols[t] felts, column-major, column c starting
 *                 c * col_stride[t] felts in (col_stride[t] >= n_rows[t]; n_rows[t] a power of two, 1 .. 2^32;
 *                 n_cols[t] >= 1); levels[t]: DEVICE pointer to the 2 n_rows[t] - 1 felts sp_commit_rows_dev wrote,
 *                 leaves first, root last.  The arrays cols, col_stride, n_rows, n_cols, levels themselves, table_of
 *                 and rows are HOST arrays (n_tables and n_open entries)
 *   opening i     row r = rows[i] of table t = table_of[i], h = log2 n_rows[t]:
 *                 values + 4 val_off[i]   n_cols[t] felts, the row's value in each column, in column order
 *                 leaves + 4 i            levels[t][r]  (leaves may be NULL: not wanted)
 *                 siblings + 4 off[i]     h felts, sibling l = levels[t][base_l + ((r >> l) ^ 1)] with
 *                                         base_l = 2 n_rows - (2 n_rows >> l); a table of one row has none
 *   val_off, off  HOST arrays of n_open + 1 entries that the call FILLS (val_off[0] = off[0] = 0), in felts
 * so (leaves, siblings, off, keys = rows) is, unchanged, the input of sp_merkle_fold_paths / sp_merkle_verify_paths.
 * Duplicated and unordered openings are legal, each answered in its own slot.  sp_commit_open_size gives the two
 * totals (felts of values, felts of siblings) from the shapes alone; it needs no device.
 * SP_ERR_BAD_ARGUMENT, before anything is launched or written, sp_last_error() naming the argument: n_tables == 0
 * with n_open > 0; a NULL table pointer (or a NULL array that is needed); n_rows of 0, not a power of two or above
 * 2^32; n_cols == 0; col_stride < n_rows (or so large that n_cols columns leave the address space); table_of[i] >=
 * n_tables; rows[i] >= n_rows; more than 2^32 - 1 value felts or sibling felts in total; a NULL required output
 * (val_off, off; values; siblings if any table has more than one row).  n_open == 0 is SP_OK with both offset
 * arrays = {0}.
 * The context is the one of the device cols[0] lives on; all tables of one call live there.  The _dev call takes
 * values, leaves and siblings on the device, enqueues on `stream` and waits for nothing; the host arrays have been
 * copied when it returns.  sp_commit_open takes them as HOST arrays: it runs on a host lane of that context and
 * brings the three back in ONE device-to-host copy through the lane's page-locked buffer (above 4 MiB: one direct
 * copy per array); the lane's stream waits for no other, so the stream that committed the tables must have drained.  One launch serves up to 65536 openings, the largest class; above that consecutive slices go out
 * on the same stream.  The launches are bracketed by sp_profile_begin / sp_profile_end (units: openings).
 * Not capturable into a graph on first use: the per-stream metadata buffer (48 bytes per table, 20 per opening) and
 * the stream's page-locked staging buffer grow on demand, as the host lane's buffers do.
 * Measured: profiles/open_queries.txt (tools/quick_open_queries.py). */
int sp_commit_open_size(size_t n_tables, const size_t* n_rows, const size_t* n_cols, size_t n_open,
                        const uint32_t* table_of, size_t* n_values, size_t* n_siblings);
int sp_commit_open_dev(size_t n_tables, const void* const* cols, const size_t* col_stride, const size_t* n_rows,
                       const size_t* n_cols, const void* const* levels, size_t n_open, const uint32_t* table_of,
                       const uint64_t* rows, uint64_t* values, uint32_t* val_off, uint64_t* leaves, uint64_t* siblings,
                       uint32_t* off, void* stream);
int sp_commit_open(size_t n_tables, const void* const* cols, const size_t* col_stride, const size_t* n_rows,
                   const size_t* n_cols, const void* const* levels, size_t n_open, const uint32_t* table_of,
                   const uint64_t* rows, uint64_t* values, uint32_t* val_off, uint64_t* leaves, uint64_t* siblings,
                   uint32_t* off);

/* Verifying a proof: the field arithmetic of a verifier of stark.prove_trace's proofs, on opened values only.  Both
 * calls take DEVICE arrays of packed felts, the challenges and the shift as HOST felts, enqueue ONE launch on
 * `stream` (one item per lane, grids from the item count alone; bracketed by sp_profile_begin / sp_profile_end) and
 * wait for nothing.  Neither builds or reads a table that grows with the trace: the periodic table has 4 * period
 * rows, and a fold item derives its own point of the coset.  A count of 0 is SP_OK without a launch; a NULL pointer
 * with a count above 0, an unknown `air`, a violated bound or a bad shift is SP_ERR_BAD_ARGUMENT before anything is
 * launched or written.  At most 2^30 items per call.
 *
 * sp_air_eval_points_dev: the composition value sum_k alpha_k C_k / Z_H at n_points LDE positions of the AIR `air`
 *   (SP_AIR_*), exactly what the dense call of that AIR (sp_air_eval_dev, sp_air_eval_ec_ladder_dev,
 *   sp_air_eval_ecdsa_dev, sp_air_eval_range_check_dev) writes at index pos[i].  log_n, periodic_lde, alphas_host
 *   and shift_host are the dense call's, with its bounds on log_n and its rule on the shift.
 *     pos[i]     LDE index below M = 4 * 2^log_n (u64)
 *     cur, nxt   n_points x n_cols felts, row-major: the trace row at pos[i] and the one at (pos[i] + 4) mod M
 *     out[i]     the value;  status[i] = SP_POINT_OK, or SP_POINT_OUT_OF_RANGE with out[i] = 0 when pos[i] >= M or
 *                a felt of the two rows is not below p (nothing is read out of bounds for any pos[i])
 * sp_fri_check_queries_dev: the fold chain of n_queries queries through n_layers committed FRI layers, layer 0 of
 *   2^log_m points on shift * <w>; 1 <= n_layers < log_m <= 32.
 *     index[q]      the query's index below 2^(log_m - 1) (u64)
 *     pairs         n_queries x n_layers x 2 felts: the two opened values of layer k, at jk = index[q] mod
 *                   2^(log_m - k - 1) and at jk + 2^(log_m - k - 1)
 *     final_layer   2^(log_m - n_layers) felts;  betas_host: n_layers felts
 *     status[q * n_layers + k]   with x = shift^(2^k) w_{2^(log_m - k)}^jk and
 *                   folded = (a + b) / 2 + beta_k (a - b) / (2 x): SP_FOLD_OK when folded equals the member
 *                   (jk < 2^(log_m - k - 2) ? 0 : 1) of the pair of layer k + 1 - final_layer[jk] after the last
 *                   layer -, SP_FOLD_MISMATCH when it does not, SP_FOLD_OUT_OF_RANGE when a, b or that value is not
 *                   below p or index[q] >= 2^(log_m - 1) (then for every layer of the query)
 * What a verifier does around them - transcript, Merkle paths, the final layer's degree - is starkperp.stark.verify. */
#define SP_AIR_PEDERSEN 0
#define SP_AIR_EC_LADDER 1
#define SP_AIR_ECDSA 2
#define SP_AIR_RANGE_CHECK 3
#define SP_POINT_OK 0
#define SP_POINT_OUT_OF_RANGE 1
#define SP_FOLD_OK 0
#define SP_FOLD_MISMATCH 1
#define SP_FOLD_OUT_OF_RANGE 2
int sp_air_eval_points_dev(int air, unsigned log_n, const uint64_t* periodic_lde, const uint64_t* alphas_host,
                           const uint64_t* shift_host, size_t n_points, const uint64_t* pos, const uint64_t* cur,
                           const uint64_t* nxt, uint64_t* out, uint8_t* status, void* stream);
int sp_fri_check_queries_dev(unsigned log_m, unsigned n_layers, const uint64_t* shift_host, const uint64_t* betas_host,
                             size_t n_queries, const uint64_t* index, const uint64_t* pairs,
                             const uint64_t* final_layer, uint8_t* status, void* stream);

/* sp_builtins_eval_points_dev: the composition value of a stark.prove_builtins proof at n_points LDE positions - the
 *   sum mod p over the present segments (`segments`: SP_SEG_* bits, 1 .. 7) of each segment's composition, bit for
 *   bit what the prover builds at index pos[i] with sp_air_eval_dev (pedersen), sp_air_eval_ecdsa_dev,
 *   sp_air_eval_rc16_dev and sp_felt_add_dev.  Same conventions as the two calls above: DEVICE arrays of packed
 *   felts, HOST challenges, ONE launch on `stream` for any count up to 2^30 (64 points per block, one wave per
 *   present segment; bracketed by sp_profile_begin / sp_profile_end with units = points), no table that grows with
 *   the trace: the rc16 part derives the coset point x = shift w_M^pos[i] and the two boundary denominators'
 *   inverses itself, where the dense call reads three tables of M felts.
 *     log_n        at least the largest minimum of the present segments (pedersen 9, ecdsa 10, rc16 3); at most 30,
 *                  24 with rc16 (the dense rc16 call's bound)
 *     per_*        the segment's stark.periodic_lde table (6 x 2048, 12 x 4096, 2 x 32 felts); NULL when absent
 *     alphas_host  11 + 26 + 8 felts of the present segments, in that order;  shift_host: the dense calls' rule
 *     z_host, rc_min, rc_max   the rc16 challenge and limb range (rc_min <= rc_max <= 0xffff, z below p); read
 *                  only with rc16, z_host may be NULL without it
 *     pos[i]       LDE index below M = 4 * 2^log_n (u64)
 *     cur, nxt     n_points x n_cols felts, row-major, n_cols = 4 + 10 + 3 of the present segments: the phase-1 row
 *                  at pos[i] and the one at (pos[i] + 4) mod M
 *     pcur, pnxt   n_points felts each: the phase-2 column at those two rows; NULL without rc16
 *     out[i]       the value;  status[i] = SP_POINT_OK, or SP_POINT_OUT_OF_RANGE with out[i] = 0 when pos[i] >= M or
 *                  one of the 2 n_cols felts - with rc16 also pcur[i], pnxt[i] - is not below p (nothing is read
 *                  out of bounds for any pos[i])
 *   SP_ERR_BAD_ARGUMENT before anything is launched or written: segments outside 1 .. 7, log_n out of range, a bad
 *   limb range or z with rc16, more than 2^30 points, a needed NULL pointer with n_points > 0, a bad shift.  A count
 *   of 0 is SP_OK without a launch.  The verifier around it is starkperp.stark.verify_builtins. */
#define SP_SEG_PEDERSEN 1
#define SP_SEG_ECDSA 2
#define SP_SEG_RC16 4
int sp_builtins_eval_points_dev(unsigned segments, unsigned log_n, const uint64_t* per_pedersen,
                                const uint64_t* per_ecdsa, const uint64_t* per_rc16, const uint64_t* alphas_host,
                                const uint64_t* shift_host, const uint64_t* z_host, uint64_t rc_min, uint64_t rc_max,
                                size_t n_points, const uint64_t* pos, const uint64_t* cur, const uint64_t* nxt,
                                const uint64_t* pcur, const uint64_t* pnxt, uint64_t* out, uint8_t* status,
                                void* stream);

/* Binding a Pedersen proof to its hashes (starkperp.stark.prove_hashes / verify_hashes).  The
 * Pedersen-step AIR says that SOME hashes were computed.  With n = 2^log_n = 512 k rows, g = w_n and X, Y, H the
 * polynomials of degree < k that take the public x_i, y_i, h_i at g^(512 i), three boundary quotients say which:
 *     B(x) = a_0 (s(x) - X(x)) / (x^k - 1) + a_1 (s(x) - Y(x g^-256)) / (x^k + 1) + a_2 (px(x) - H(x g^-511)) / (x^k - g^-k)
 * (s at row 512 i is x_i, s at row 512 i + 256 is y_i, px at row 512 i + 511 is h_i).  Conventions are those of
 * sp_air_eval_dev and sp_air_eval_points_dev: DEVICE arrays of packed felts, the three challenges and the shift as
 * HOST felts, enqueued on `stream`, nothing waited for, the shift neither 0 nor a felt with shift^(4n) = 1 (no
 * denominator vanishes on such a coset), SP_ERR_BAD_ARGUMENT - sp_last_error() naming the call and the argument -
 * before anything is launched or written.  The launches of a call are bracketed by sp_profile_begin / sp_profile_end
 * as one entry (units = points).
 *
 * sp_hash_io_boundary_dev: out[j] = (acc ? acc[j] : 0) + B(x_j) mod p for every j < M = 4 n, x_j = shift w_M^j.
 *     trace_lde    the committed trace LDE, columns col_stride >= M felts apart; only columns 0 (s) and 1 (px) are read
 *     pub_lde      3 columns of M felts: X, Y, H at x_j, x_j g^-256 and x_j g^-511 - three sp_lde_dev calls of k points
 *                  at log_blowup 11 with the shifts shift, shift g^-256, shift g^-511
 *     acc          NULL, or M felts; may be `out`
 *     log_n        9 .. 24, the range in which sp_lde_dev can produce pub_lde
 *   x_j^k = shift^k w_2048^j takes 2048 values whatever n is: the call inverts the 3 x 2048 denominators itself, 16
 *   behind one inversion, into a 192 KiB table per stream - it allocates nothing that grows with M - and then runs
 *   ONE elementwise launch, seven felts moved and one field reduction per point.
 * sp_hash_io_boundary_points_dev: B at n_points LDE positions, canonically what the dense call adds at index pos[i].
 *     coef         3 x k felts: the coefficients of X, Y, H in natural order - sp_ntt_dev(inverse = 1) of the three
 *                  public columns
 *     pos[i]       LDE index below M (u64);  cur: n_points x 4 felts, the opened trace row at pos[i]
 *     out[i]       the value;  status[i] = SP_POINT_OK, or SP_POINT_OUT_OF_RANGE with out[i] = 0 when pos[i] >= M or
 *                  a felt of the row is not below p (nothing is read out of bounds for any pos[i])
 *     log_n        9 .. 30;  n_points at most 2^30, 0 is SP_OK without a launch
 *   One block of 256 lanes per point, the same plan for every k from 1 up: every lane derives x = shift w_M^pos[i] by
 *   square-and-multiply, takes the coefficients lane, lane + 256, ... of each polynomial by Horner in y^256, scales by
 *   y^lane; a tree in LDS adds the shares and lane 0 inverts the product of the three denominators once.  About
 *   3 k / 256 multiplications per lane: nothing proportional to M is built or read. */
int sp_hash_io_boundary_dev(const uint64_t* trace_lde, size_t col_stride, const uint64_t* pub_lde, unsigned log_n,
                            const uint64_t* alphas_host, const uint64_t* shift_host, const uint64_t* acc, uint64_t* out,
                            void* stream);
int sp_hash_io_boundary_points_dev(unsigned log_n, const uint64_t* coef, const uint64_t* alphas_host,
                                   const uint64_t* shift_host, size_t n_points, const uint64_t* pos, const uint64_t* cur,
                                   uint64_t* out, uint8_t* status, void* stream);

/* Boundary constraints from a descriptor (starkperp.stark.prove_signatures / verify_signatures,
 * prove_ranges / verify_ranges).  The machinery of the hash-io pair above for ANY periodic AIR: period p =
 * 2^log_period, n = 2^log_n = p k rows, g = w_n, omega = g^p of order k, M = 4 n.  The descriptor, HOST arrays read
 * before the call returns, names boundary GROUPS - a row o_d below the period each - and TERMS (column c_t, group):
 * "column c_t at row p i + o_d is v_t[i]" for a public list v_t.  With one challenge a_t per term and C_d the
 * polynomial of degree < k through sum_{t in d} a_t v_t[i] at omega^i (one public polynomial per GROUP, combined by
 * the caller before any extension),
 *     B(x) = sum_d ( sum_{t in d} a_t col_{c_t}(x) - C_d(x g^-o_d) ) / (x^k - w_p^o_d).
 *     log_period   7 .. 10          n_cols   1 .. 16, the columns of the trace (and of an opened row)
 *     n_groups     1 .. 4;  group_rows[n_groups] distinct and below p
 *     n_terms      1 .. 8;  term_cols[t] < n_cols, term_groups[t] < n_groups, every group with at least one term
 *   The ECDSA AIR is {10, 10, 3, {0, 256, 512}, 5, {0, 0, 3, 4, 0}, {0, 1, 1, 1, 2}}, the range-check AIR
 *   {7, 1, 1, {0}, 1, {0}, {0}}, and {9, 4, 3, {0, 256, 511}, 3, {0, 0, 1}, {0, 1, 2}} is the hash-io pair: with it
 *   and pub_lde / coef scaled by the challenges the calls below return what those return, bit for bit.
 * Conventions are those of the hash-io pair: DEVICE arrays of packed felts, the n_terms challenges (in the
 * descriptor's term order) and the shift as HOST felts, enqueued on `stream`, nothing waited for, the shift neither 0
 * nor a felt with shift^(4n) = 1, SP_ERR_BAD_ARGUMENT - sp_last_error() naming the call and the argument - before
 * anything is launched or written.  The launches of a call are bracketed by sp_profile_begin / sp_profile_end as one
 * entry (units = points).
 *
 * sp_boundary_dev: out[j] = (acc ? acc[j] : 0) + B(x_j) mod p for every j < M, x_j = shift w_M^j.
 *     trace_lde    the committed trace LDE, columns col_stride >= M felts apart; only the terms' columns are read
 *     pub_lde      n_groups columns of M felts: C_d at x_j g^-o_d - one sp_lde_dev call per group, k points at
 *                  log_blowup log_period + 2 with the shift shift g^-o_d
 *     acc          NULL, or M felts; may be `out`
 *     log_n        log_period .. 24, the range in which sp_lde_dev can produce pub_lde
 *   x_j^k = shift^k w_4p^j takes 4 p values whatever n is: the call inverts the n_groups x 4p denominators itself, 16
 *   behind one inversion, into a table per stream (n_groups * 4p felts: 384 KiB for the ECDSA descriptor) - it
 *   allocates nothing that grows with M - and then runs ONE elementwise launch: n_terms + 2 n_groups + 1 (+ 1)
 *   felts moved per point, at most three products behind each field reduction.
 * sp_boundary_points_dev: B at n_points LDE positions, canonically what the dense call adds at index pos[i].
 *     coef         n_groups x k felts: the coefficients of the C_d in natural order - sp_ntt_dev(inverse = 1) of the
 *                  combined public columns
 *     pos[i]       LDE index below M (u64);  cur: n_points x n_cols felts, the opened trace row at pos[i]
 *     out[i]       the value;  status[i] = SP_POINT_OK, or SP_POINT_OUT_OF_RANGE with out[i] = 0 when pos[i] >= M or
 *                  a felt of the row is not below p (nothing is read out of bounds for any pos[i])
 *     log_n        log_period .. 30;  n_points at most 2^30, 0 is SP_OK without a launch
 *   One block of 256 lanes per point, the same plan for every k from 1 up: every lane derives x = shift w_M^pos[i] by
 *   square-and-multiply, takes the coefficients lane, lane + 256, ... of each C_d by Horner in y^256, scales by
 *   y^lane; a tree in LDS (36 KiB) adds the shares and lane 0 inverts the product of the denominators once. */
int sp_boundary_dev(unsigned log_period, unsigned n_cols, unsigned n_groups, const unsigned* group_rows,
                    unsigned n_terms, const unsigned* term_cols, const unsigned* term_groups, const uint64_t* trace_lde,
                    size_t col_stride, const uint64_t* pub_lde, unsigned log_n, const uint64_t* alphas_host,
                    const uint64_t* shift_host, const uint64_t* acc, uint64_t* out, void* stream);
int sp_boundary_points_dev(unsigned log_period, unsigned n_cols, unsigned n_groups, const unsigned* group_rows,
                           unsigned n_terms, const unsigned* term_cols, const unsigned* term_groups, unsigned log_n,
                           const uint64_t* coef, const uint64_t* alphas_host, const uint64_t* shift_host,
                           size_t n_points, const uint64_t* pos, const uint64_t* cur, uint64_t* out, uint8_t* status,
                           void* stream);

/* Boundary constraints of the builtins proof (starkperp.stark.prove_builtin_usage /
 * verify_builtin_usage).  The combined builtin trace lays the present segments (`segments`: SP_SEG_* bits, 1 .. 7)
 * side by side - 4 + 10 + 3 columns - each with its own period p_s (512, 1024, 8) and k_s = n / p_s instances.  Every
 * segment brings the groups and terms of a descriptor of the pair above, columns relative to its first column:
 *     pedersen   {9, 4, 3, {0, 256, 511}, 3, {0, 0, 1}, {0, 1, 2}}                 s = x | s = y | px = h
 *     ecdsa      {10, 10, 3, {0, 256, 512}, 5, {0, 0, 3, 4, 0}, {0, 1, 1, 1, 2}}   m = z | m = r, qx, qy | m = w
 *     rc16       {3, 3, 1, {7}, 1, {1}, {0}}                                       acc = value_i at row 8 i + 7
 * and B(x) is the sum over ALL 3 + 3 + 1 groups of the quotient above, each with its own segment's p and k.  The
 * 3 + 5 + 1 challenges stand in segment order.  Conventions are those of the pair above: DEVICE arrays of packed
 * felts, HOST challenges and shift, enqueued on `stream`, nothing waited for, SP_ERR_BAD_ARGUMENT - sp_last_error()
 * naming the call and the argument - before anything is launched or written, the launches of a call bracketed by
 * sp_profile_begin / sp_profile_end as one entry (units = points, for the combine call items).
 *
 * sp_boundary_combine_dev: the public columns before extension, out[d][i] = sum_{t in d} a_t v_t[i] mod p, canonical,
 *   for i < k - what every caller of the pair above does "before any extension", here on the device.
 *     n_groups 1 .. 4, n_terms 1 .. 8, term_groups[t] < n_groups with every group used (host array)
 *     values_host  HOST array of n_terms DEVICE columns of k felts each (any 256-bit value), in term order
 *     alphas_host  n_terms felts;  k  1 .. 2^30;  out  n_groups x k felts, no column of values_host
 *   One launch, one item per lane, at most three products behind a reduction.
 * sp_builtins_boundary_dev: out[j] = (acc ? acc[j] : 0) + B(x_j) mod p for every j < M = 4 * 2^log_n.
 *     trace_lde    the committed phase-1 LDE: the 4 + 10 + 3 columns of the present segments, col_stride >= M apart
 *     pub_lde      3 + 3 + 1 columns of M felts, the present segments' groups in order: C_d at x_j g^-o_d - one
 *                  sp_lde_dev call per group, k_s points at log_blowup log_period_s + 2 with the shift shift g^-o_d
 *     alphas_host  3 + 5 + 1 felts of the present segments;  acc  NULL, or M felts; may be `out`
 *     log_n        the largest minimum of the present segments (9, 10, 3) .. 24;  shift_host: the pair's rule
 *   ONE table-build launch writes every group's 4 p_s inverse denominators into a per-stream table (at most 3 * 2048 +
 *   3 * 4096 + 32 felts, nothing that grows with M), ONE elementwise launch follows, one point per lane.  With one
 *   segment the result is sp_boundary_dev's with that descriptor, bit for bit.
 * sp_builtins_boundary_points_dev: B at n_points LDE positions, canonically what the dense call adds at index pos[i].
 *     coef         the groups' coefficient arrays back to back, natural order: 3 k_pedersen, 3 k_ecdsa, k_rc16 felts -
 *                  sp_ntt_dev(inverse = 1) of the combined public columns
 *     pos[i]       LDE index below M (u64);  cur: n_points x n_cols felts, the WHOLE opened phase-1 row at pos[i]
 *     out[i]       the value;  status[i] = SP_POINT_OK, or SP_POINT_OUT_OF_RANGE with out[i] = 0 when pos[i] >= M or
 *                  any felt of the row is not below p (nothing is read out of bounds for any pos[i])
 *     log_n        from the same minimum up to 30, 24 with rc16 (sp_builtins_eval_points_dev's bound);  n_points at
 *                  most 2^30, 0 is SP_OK without a launch
 *   ONE launch, one block of 256 lanes per point; the segments run one after the other through the same 36 KiB of
 *   LDS, each as sp_boundary_points_dev runs its descriptor, and lane 0 keeps the running sum.  About
 *   sum_d k_d / 256 multiplications per lane: with rc16 at n = 2^23 that is 4096 Horner steps. */
int sp_boundary_combine_dev(unsigned n_groups, unsigned n_terms, const unsigned* term_groups,
                            const uint64_t* const* values_host, size_t k, const uint64_t* alphas_host, uint64_t* out,
                            void* stream);
int sp_builtins_boundary_dev(unsigned segments, unsigned log_n, const uint64_t* trace_lde, size_t col_stride,
                             const uint64_t* pub_lde, const uint64_t* alphas_host, const uint64_t* shift_host,
                             const uint64_t* acc, uint64_t* out, void* stream);
int sp_builtins_boundary_points_dev(unsigned segments, unsigned log_n, const uint64_t* coef, const uint64_t* alphas_host,
                                    const uint64_t* shift_host, size_t n_points, const uint64_t* pos, const uint64_t* cur,
                                    uint64_t* out, uint8_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* STARKPERP_H */
