// Keccak Merkle tree over field elements (merkle_tree/src/merkle_tree.rs), C ABI:
// the tree in device memory, every hash on the GPU (merkle.hpp); the host
// side holds the reference's checks and the host-only hash / proof check.
#include "host.hpp"
#include "hfield.hpp"
#include "merkle.hpp"

using namespace zkh;

struct zk_merkle {
  zk_ctx* c = nullptr;
  zk_field field = ZK_BN254_FR;
  uint32_t depth = 0;
  uint64_t N = 0;      // leaves
  Fe* tree = nullptr;  // leaves, then the levels back to back (merkle.hpp), canonical
  DevBuf ids, data, flags, gat;  // staging of the batched calls (grow-only)
};

namespace {
// what the device can at most be asked for: (2^(depth+1) - 1) * 32 B
constexpr uint32_t kMaxDepth = 40;

// ---- host hashing (zk::Keccak256 + hfield.hpp) ----
template <class F>
Fe h_digest_mod_p(const uint8_t (&d)[32]) {  // from_le_bytes_mod_order
  Fe x;
  memcpy(x.v, d, 32);
  return zk::h64::fe(zk::h64::reduce<F>(zk::h64::of(x)));
}
template <class F>
Fe h_hash_leaf(const Fe& x) {  // compute_hash :201-206 (canonical in, canonical out)
  uint8_t d[32];
  zk::Keccak256 h;
  h.update(reinterpret_cast<const uint8_t*>(x.v), 32);
  h.finalize_reset(d);
  return h_digest_mod_p<F>(d);
}
template <class F>
Fe h_hash_pair(const Fe& l, const Fe& r) {  // hash_pair :208-214
  uint8_t d[32];
  zk::Keccak256 h;
  h.update(reinterpret_cast<const uint8_t*>(l.v), 32);
  h.update(reinterpret_cast<const uint8_t*>(r.v), 32);
  h.finalize_reset(d);
  return h_digest_mod_p<F>(d);
}
// host scalar in -> canonical (checked < p), canonical -> host scalar out
template <class F>
Fe in_canon(zk_repr repr, const zk_fe& a) {
  const Fe x = from_zk(a);
  require(zk::fe_is_canonical<F>(x), "field element >= modulus");
  return repr == ZK_REPR_MONTGOMERY ? zk::hfe_from_mont<F>(x) : x;
}
template <class F>
zk_fe out_canon(zk_repr repr, const Fe& c) {
  return to_zk(repr == ZK_REPR_MONTGOMERY ? zk::hfe_to_mont<F>(c) : c);
}

// ---- launches: on the context's stream, no stats kind of their own ----
template <class K>
uint32_t merkle_grid(zk_ctx* c, uint64_t work, K kernel) {
  uint32_t g = grid_for(c, work, kernel);
  if (c->grid_cap > 0 && g > c->grid_cap) g = c->grid_cap;
  return g;
}
#define MERKLE_LAUNCH(c, kernel, grid, ...)                                  \
  do {                                                                       \
    kernel<<<dim3(grid), dim3(zk::kBlock), 0, (c)->stream>>>(__VA_ARGS__);   \
    HIPCK(hipGetLastError());                                                \
  } while (0)

// tree[0 .. depth-1] from the leaves: one kernel per wide level, then the
// levels of at most kBlock nodes in one block (k_merkle_top)
template <class F>
void build_levels(zk_merkle* m) {
  zk_ctx* c = m->c;
  int l0 = 0;
  while ((m->N >> (l0 + 1)) > (uint64_t)zk::kBlock) ++l0;
  for (int l = 0; l < l0; ++l) {
    const uint64_t np = m->N >> (l + 1);
    const uint32_t grid = merkle_grid(c, np, zk::k_merkle_level<F>);
    MERKLE_LAUNCH(c, zk::k_merkle_level<F>, grid, m->tree + zk::merkle_level_off(m->N, l - 1),
                  m->tree + zk::merkle_level_off(m->N, l), np);
  }
  MERKLE_LAUNCH(c, zk::k_merkle_top<F>, 1, m->tree, m->N, l0, (int)m->depth);
}

struct TreeGuard {  // frees a half-built tree on an error path
  zk_merkle* m;
  ~TreeGuard() {
    if (!m) return;
    if (m->tree) (void)hipFree(m->tree);
    delete m;
  }
};

// Montgomery (FromMont) or canonical inputs already at d_in, checked < p
template <class F>
zk_merkle* tree_from_device(zk_ctx* c, zk_field field, uint32_t depth, const Fe* d_in, uint64_t n_inputs, bool from_mont) {
  TreeGuard g{new zk_merkle};
  zk_merkle* m = g.m;
  m->c = c;
  m->field = field;
  m->depth = depth;
  m->N = (uint64_t)1 << depth;
  const size_t bytes = (size_t)(2 * m->N - 1) * sizeof(Fe);
  if (hipMalloc(reinterpret_cast<void**>(&m->tree), bytes) != hipSuccess) {
    (void)hipGetLastError();
    m->tree = nullptr;
    fail(ZK_EDEVICE, "merkle tree: hipMalloc of " + std::to_string(bytes) + " bytes failed");
  }
  if (from_mont) {
    const auto kern = zk::k_merkle_leaves<F, true>;
    MERKLE_LAUNCH(c, kern, merkle_grid(c, m->N, kern), d_in, n_inputs, m->tree, m->N);
  } else {
    const auto kern = zk::k_merkle_leaves<F, false>;
    MERKLE_LAUNCH(c, kern, merkle_grid(c, m->N, kern), d_in, n_inputs, m->tree, m->N);
  }
  build_levels<F>(m);
  sync(c);
  g.m = nullptr;
  return m;
}

void check_shape(zk_ctx* c, uint32_t depth, uint64_t n_inputs, zk_merkle** out) {
  require(c && out, "null argument");
  require(depth >= 1, "merkle tree: depth 0 has no root (get_root_hash indexes tree[depth - 1])");
  if (depth > kMaxDepth) fail(ZK_EDEVICE, "merkle tree: a tree of this depth cannot be allocated");
  require(n_inputs <= ((uint64_t)1 << depth), "Too many inputs for tree depth");
}

void ids_in_range(const zk_merkle* m, const uint64_t* ids, size_t n) {
  for (size_t i = 0; i < n; ++i) require(ids[i] < m->N, "Invalid leaf ID");
}
}  // namespace

extern "C" {

int zk_merkle_new(zk_ctx* c, zk_field field, uint32_t depth, zk_repr repr, const zk_fe* inputs, uint64_t n_inputs,
                  zk_merkle** out) {
  return guarded([&] {
    check_shape(c, depth, n_inputs, out);
    require(n_inputs == 0 || inputs, "null argument");
    require(repr == ZK_REPR_CANONICAL || repr == ZK_REPR_MONTGOMERY, "unknown representation");
    bind(c);
    dispatch(field, [&](auto f) {
      using F = decltype(f);
      // staged as given (no conversion): upload's check that every value is < p
      c->input.ensure(std::max<uint64_t>(n_inputs, 1) * 32);
      upload<F>(c, ZK_REPR_MONTGOMERY, inputs, n_inputs, c->input.fe());
      *out = tree_from_device<F>(c, field, depth, c->input.fe(), n_inputs, repr == ZK_REPR_MONTGOMERY);
    });
  });
}

int zk_dev_merkle_new(zk_ctx* c, zk_field field, uint32_t depth, const void* dev_inputs, uint64_t n_inputs,
                      zk_merkle** out) {
  return guarded([&] {
    check_shape(c, depth, n_inputs, out);
    require(n_inputs == 0 || dev_inputs, "null argument");
    bind(c);
    dispatch(field, [&](auto f) {
      using F = decltype(f);
      const Fe* d_in = reinterpret_cast<const Fe*>(dev_inputs);
      if (n_inputs > 0) {
        HIPCK(hipMemsetAsync(d_flag(c), 0, 4, c->stream));
        MERKLE_LAUNCH(c, zk::k_check_canonical<F>, merkle_grid(c, n_inputs, zk::k_check_canonical<F>), d_in, n_inputs,
                      d_flag(c));
        uint32_t bad = 0;
        HIPCK(hipMemcpyAsync(&bad, d_flag(c), 4, hipMemcpyDeviceToHost, c->stream));
        sync(c);
        require(bad == 0, "field element >= modulus in input table");
      }
      *out = tree_from_device<F>(c, field, depth, d_in, n_inputs, true);
    });
  });
}

void zk_merkle_free(zk_merkle* m) {
  if (!m) return;
  if (m->c) (void)hipSetDevice(m->c->device);
  if (m->tree) (void)hipFree(m->tree);
  m->ids.release();
  m->data.release();
  m->flags.release();
  m->gat.release();
  delete m;
}

int zk_merkle_root(zk_merkle* m, zk_repr repr, zk_fe* out) {
  return guarded([&] {
    require(m && out, "null argument");
    zk_ctx* c = m->c;
    bind(c);
    Fe r;
    HIPCK(hipMemcpyAsync(&r, m->tree + zk::merkle_level_off(m->N, (int)m->depth - 1), sizeof r, hipMemcpyDeviceToHost,
                         c->stream));
    sync(c);
    dispatch(m->field, [&](auto f) { *out = out_canon<decltype(f)>(repr, r); });
  });
}

int zk_merkle_download(zk_merkle* m, int level, zk_repr repr, zk_fe* out) {
  return guarded([&] {
    require(m && out, "null argument");
    require(level >= -1 && level < (int)m->depth, "merkle tree: no such level");
    zk_ctx* c = m->c;
    bind(c);
    const uint64_t w = m->N >> (level + 1);
    HIPCK(hipMemcpyAsync(out, m->tree + zk::merkle_level_off(m->N, level), w * sizeof(Fe), hipMemcpyDeviceToHost,
                         c->stream));
    sync(c);
    if (repr == ZK_REPR_MONTGOMERY)
      dispatch(m->field, [&](auto f) {
        for (uint64_t i = 0; i < w; ++i) out[i] = to_zk(zk::hfe_to_mont<decltype(f)>(from_zk(out[i])));
      });
  });
}

int zk_merkle_update_leaves(zk_merkle* m, zk_repr repr, const uint64_t* ids, const zk_fe* data, const uint8_t* is_hash,
                            size_t n) {
  return guarded([&] {
    require(m, "null argument");
    if (n == 0) return;
    require(ids && data && is_hash, "null argument");
    require(repr == ZK_REPR_CANONICAL || repr == ZK_REPR_MONTGOMERY, "unknown representation");
    ids_in_range(m, ids, n);
    {
      std::vector<uint64_t> s(ids, ids + n);
      std::sort(s.begin(), s.end());
      require(std::adjacent_find(s.begin(), s.end()) == s.end(),
              "merkle update: duplicate leaf id (the reference applies updates one after another)");
    }
    zk_ctx* c = m->c;
    bind(c);
    dispatch(m->field, [&](auto f) {
      using F = decltype(f);
      m->data.ensure(n * 32);
      m->ids.ensure(n * 8);
      m->flags.ensure(n);
      upload<F>(c, ZK_REPR_MONTGOMERY, data, n, m->data.fe());  // as given, checked < p; nothing written before
      uint64_t* d_ids = reinterpret_cast<uint64_t*>(m->ids.p);
      uint8_t* d_fl = reinterpret_cast<uint8_t*>(m->flags.p);
      HIPCK(hipMemcpyAsync(d_ids, ids, n * 8, hipMemcpyHostToDevice, c->stream));
      HIPCK(hipMemcpyAsync(d_fl, is_hash, n, hipMemcpyHostToDevice, c->stream));
      if (repr == ZK_REPR_MONTGOMERY) {
        const auto kern = zk::k_merkle_set_leaves<F, true>;
        MERKLE_LAUNCH(c, kern, merkle_grid(c, n, kern), m->tree, d_ids, m->data.fe(), d_fl, (uint64_t)n);
      } else {
        const auto kern = zk::k_merkle_set_leaves<F, false>;
        MERKLE_LAUNCH(c, kern, merkle_grid(c, n, kern), m->tree, d_ids, m->data.fe(), d_fl, (uint64_t)n);
      }
      const uint32_t grid = merkle_grid(c, n, zk::k_merkle_update_level<F>);
      for (int l = 0; l < (int)m->depth; ++l)  // level by level: shared ancestors see final children
        MERKLE_LAUNCH(c, zk::k_merkle_update_level<F>, grid, m->tree, m->N, l, d_ids, (uint64_t)n);
      sync(c);
    });
  });
}

int zk_merkle_create_proofs(zk_merkle* m, zk_repr repr, const zk_fe* data, const uint64_t* ids, size_t n,
                            zk_fe* out_siblings, uint8_t* out_sides) {
  return guarded([&] {
    require(m, "null argument");
    if (n == 0) return;
    require(data && ids && out_siblings && out_sides, "null argument");
    require(repr == ZK_REPR_CANONICAL || repr == ZK_REPR_MONTGOMERY, "unknown representation");
    ids_in_range(m, ids, n);
    zk_ctx* c = m->c;
    bind(c);
    dispatch(m->field, [&](auto f) {
      using F = decltype(f);
      const uint64_t per = (uint64_t)m->depth + 1;
      std::vector<Fe> want(n), got(n * per);
      for (size_t i = 0; i < n; ++i) want[i] = h_hash_leaf<F>(in_canon<F>(repr, data[i]));
      m->ids.ensure(n * 8);
      m->gat.ensure(got.size() * sizeof(Fe));
      uint64_t* d_ids = reinterpret_cast<uint64_t*>(m->ids.p);
      HIPCK(hipMemcpyAsync(d_ids, ids, n * 8, hipMemcpyHostToDevice, c->stream));
      MERKLE_LAUNCH(c, zk::k_merkle_gather, merkle_grid(c, got.size(), zk::k_merkle_gather), m->tree, m->N,
                    (int)m->depth, d_ids, (uint64_t)n, m->gat.fe());
      HIPCK(hipMemcpyAsync(got.data(), m->gat.p, got.size() * sizeof(Fe), hipMemcpyDeviceToHost, c->stream));
      sync(c);
      for (size_t i = 0; i < n; ++i)  // :149-151, all or nothing
        require(zk::fe_eq<F>(got[i * per], want[i]), "Data does not match the leaf hash");
      for (size_t i = 0; i < n; ++i)
        for (uint32_t lev = 0; lev < m->depth; ++lev) {
          out_siblings[i * m->depth + lev] = out_canon<F>(repr, got[i * per + 1 + lev]);
          out_sides[i * m->depth + lev] = ((ids[i] >> lev) & 1) ? 0 : 1;  // even index: LeafSide::Right :165-169
        }
    });
  });
}

// ---- host only ----
int zk_merkle_hash_leaf(zk_field field, zk_repr repr, const zk_fe* x, zk_fe* out) {
  return guarded([&] {
    require(x && out, "null argument");
    require(repr == ZK_REPR_CANONICAL || repr == ZK_REPR_MONTGOMERY, "unknown representation");
    dispatch(field, [&](auto f) {
      using F = decltype(f);
      *out = out_canon<F>(repr, h_hash_leaf<F>(in_canon<F>(repr, *x)));
    });
  });
}

int zk_merkle_hash_pair(zk_field field, zk_repr repr, const zk_fe* left, const zk_fe* right, zk_fe* out) {
  return guarded([&] {
    require(left && right && out, "null argument");
    require(repr == ZK_REPR_CANONICAL || repr == ZK_REPR_MONTGOMERY, "unknown representation");
    dispatch(field, [&](auto f) {
      using F = decltype(f);
      *out = out_canon<F>(repr, h_hash_pair<F>(in_canon<F>(repr, *left), in_canon<F>(repr, *right)));
    });
  });
}

int zk_merkle_verify_proof(zk_field field, zk_repr repr, const zk_fe* root, const zk_fe* data, const zk_fe* siblings,
                           const uint8_t* sides, size_t len, int* out_ok) {
  return guarded([&] {
    require(root && data && out_ok && (len == 0 || (siblings && sides)), "null argument");
    require(repr == ZK_REPR_CANONICAL || repr == ZK_REPR_MONTGOMERY, "unknown representation");
    for (size_t i = 0; i < len; ++i) require(sides[i] <= 1, "merkle proof: a side is 0 (Left) or 1 (Right)");
    dispatch(field, [&](auto f) {
      using F = decltype(f);
      const Fe want = in_canon<F>(repr, *root);
      for (size_t i = 0; i < len; ++i) (void)in_canon<F>(repr, siblings[i]);  // every value < p before any work
      Fe cur = h_hash_leaf<F>(in_canon<F>(repr, *data));
      for (size_t i = 0; i < len; ++i) {  // :189-196
        const Fe s = in_canon<F>(repr, siblings[i]);
        cur = sides[i] == 0 ? h_hash_pair<F>(s, cur) : h_hash_pair<F>(cur, s);
      }
      *out_ok = zk::fe_eq<F>(cur, want) ? 1 : 0;
    });
  });
}

}  // extern "C"
