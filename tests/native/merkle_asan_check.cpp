// Sanitizer driver for the host half of the Merkle tree (test infrastructure,
// not the product): built by `make -C zk-research-implementations_amd
// asan-merkle` against the same host-only -fsanitize=address,undefined objects
// as host_asan_check, and run by tests/test_merkle_sanitizers_cpu.py on a
// machine without a GPU. It drives the three host-only entry points
// (zk_merkle_hash_leaf, zk_merkle_hash_pair, zk_merkle_verify_proof) on valid
// and hostile inputs, and zk_merkle_new / the tree calls without a device,
// which must fail cleanly. Exit status 0 and "merkle_asan_check ok" on success.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "zk_sumcheck.h"

static int failures = 0;
#define EXPECT(c)                                                   \
  do {                                                              \
    if (!(c)) {                                                     \
      fprintf(stderr, "%s:%d: expectation failed: %s\n", __FILE__, __LINE__, #c); \
      ++failures;                                                   \
    }                                                               \
  } while (0)

static uint64_t rng_state = 0x243f6a8885a308d3ull;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
static zk_fe small_fe() {  // canonical in every field (< 2^250)
  zk_fe x;
  for (int i = 0; i < 4; ++i) x.limb[i] = rnd();
  x.limb[3] &= 0x03ffffffffffffffull;
  return x;
}
static zk_fe all_ones() {  // 2^256 - 1: >= p in every field
  zk_fe x;
  for (int i = 0; i < 4; ++i) x.limb[i] = ~0ull;
  return x;
}
static bool same(const zk_fe& a, const zk_fe& b) { return memcmp(&a, &b, sizeof a) == 0; }

// a whole tree through the host entry points, an opening of every leaf, and its check
static void valid_proofs(zk_field field, zk_repr repr, unsigned depth) {
  const size_t n = (size_t)1 << depth;
  std::vector<zk_fe> data(n);
  std::vector<std::vector<zk_fe>> lv(depth + 1);
  lv[0].resize(n);
  for (size_t i = 0; i < n; ++i) {
    // inputs in `repr`: a value < 2^250 is a valid image in either representation
    data[i] = small_fe();
    EXPECT(zk_merkle_hash_leaf(field, repr, &data[i], &lv[0][i]) == ZK_OK);
  }
  for (unsigned l = 1; l <= depth; ++l) {
    lv[l].resize(n >> l);
    for (size_t j = 0; j < lv[l].size(); ++j)
      EXPECT(zk_merkle_hash_pair(field, repr, &lv[l - 1][2 * j], &lv[l - 1][2 * j + 1], &lv[l][j]) == ZK_OK);
  }
  const zk_fe root = lv[depth][0];
  for (size_t leaf = 0; leaf < n; ++leaf) {
    std::vector<zk_fe> sib(depth);
    std::vector<uint8_t> side(depth);
    size_t idx = leaf;
    for (unsigned l = 0; l < depth; ++l, idx >>= 1) {
      sib[l] = lv[l][idx ^ 1];
      side[l] = (idx & 1) ? 0 : 1;
    }
    int ok = -1;
    EXPECT(zk_merkle_verify_proof(field, repr, &root, &data[leaf], sib.data(), side.data(), depth, &ok) == ZK_OK && ok == 1);
    side[depth / 2] ^= 1;
    EXPECT(zk_merkle_verify_proof(field, repr, &root, &data[leaf], sib.data(), side.data(), depth, &ok) == ZK_OK && ok == 0);
    side[depth / 2] ^= 1;
    sib[0].limb[0] ^= 1;
    EXPECT(zk_merkle_verify_proof(field, repr, &root, &data[leaf], sib.data(), side.data(), depth, &ok) == ZK_OK && ok == 0);
    sib[0].limb[0] ^= 1;
    // a shorter proof folds to an inner node, not to the root
    EXPECT(zk_merkle_verify_proof(field, repr, &root, &data[leaf], sib.data(), side.data(), depth - 1, &ok) == ZK_OK && ok == 0);
    EXPECT(zk_merkle_verify_proof(field, repr, &lv[depth - 1][leaf >> (depth - 1)], &data[leaf], sib.data(), side.data(),
                                  depth - 1, &ok) == ZK_OK && ok == 1);
  }
}

static void hostile_inputs(zk_field field, zk_repr repr) {
  const zk_fe x = small_fe(), y = small_fe(), big = all_ones();
  zk_fe out = x;
  const zk_fe kept = out;
  int ok = -5;
  // values >= p
  EXPECT(zk_merkle_hash_leaf(field, repr, &big, &out) == ZK_EINVAL);
  EXPECT(zk_merkle_hash_pair(field, repr, &big, &y, &out) == ZK_EINVAL);
  EXPECT(zk_merkle_hash_pair(field, repr, &x, &big, &out) == ZK_EINVAL);
  // null inputs / outputs, unknown field
  EXPECT(zk_merkle_hash_leaf(field, repr, nullptr, &out) == ZK_EINVAL);
  EXPECT(zk_merkle_hash_leaf(field, repr, &x, nullptr) == ZK_EINVAL);
  EXPECT(zk_merkle_hash_pair(field, repr, &x, nullptr, &out) == ZK_EINVAL);
  EXPECT(zk_merkle_hash_pair(field, repr, nullptr, &y, &out) == ZK_EINVAL);
  EXPECT(zk_merkle_hash_pair(field, repr, &x, &y, nullptr) == ZK_EINVAL);
  EXPECT(zk_merkle_hash_leaf((zk_field)3, repr, &x, &out) == ZK_EINVAL);  // (3: the largest value the enum can hold)
  EXPECT(same(out, kept));

  zk_fe sib[3] = {small_fe(), small_fe(), small_fe()};
  uint8_t side[3] = {0, 1, 0};
  // length 0: no entries are read (null arrays allowed); the data's hash is the root or it is not
  zk_fe leaf;
  EXPECT(zk_merkle_hash_leaf(field, repr, &x, &leaf) == ZK_OK);
  EXPECT(zk_merkle_verify_proof(field, repr, &leaf, &x, nullptr, nullptr, 0, &ok) == ZK_OK && ok == 1);
  EXPECT(zk_merkle_verify_proof(field, repr, &y, &x, sib, side, 0, &ok) == ZK_OK && ok == 0);
  ok = -5;
  // a huge len with nothing behind it
  EXPECT(zk_merkle_verify_proof(field, repr, &leaf, &x, nullptr, nullptr, ~(size_t)0, &ok) == ZK_EINVAL);
  EXPECT(zk_merkle_verify_proof(field, repr, &leaf, &x, sib, nullptr, (size_t)1 << 62, &ok) == ZK_EINVAL);
  EXPECT(zk_merkle_verify_proof(field, repr, &leaf, &x, nullptr, side, (size_t)1 << 62, &ok) == ZK_EINVAL);
  // sides other than 0 / 1
  for (int bad : {2, 3, 0x80, 0xff}) {
    uint8_t s2[3] = {0, 1, (uint8_t)bad};
    EXPECT(zk_merkle_verify_proof(field, repr, &leaf, &x, sib, s2, 3, &ok) == ZK_EINVAL);
  }
  // values >= p: root, data, any sibling
  EXPECT(zk_merkle_verify_proof(field, repr, &big, &x, sib, side, 3, &ok) == ZK_EINVAL);
  EXPECT(zk_merkle_verify_proof(field, repr, &leaf, &big, sib, side, 3, &ok) == ZK_EINVAL);
  for (int k = 0; k < 3; ++k) {
    zk_fe s2[3] = {sib[0], sib[1], sib[2]};
    s2[k] = big;
    EXPECT(zk_merkle_verify_proof(field, repr, &leaf, &x, s2, side, 3, &ok) == ZK_EINVAL);
  }
  // null root / data / output
  EXPECT(zk_merkle_verify_proof(field, repr, nullptr, &x, sib, side, 3, &ok) == ZK_EINVAL);
  EXPECT(zk_merkle_verify_proof(field, repr, &leaf, nullptr, sib, side, 3, &ok) == ZK_EINVAL);
  EXPECT(zk_merkle_verify_proof(field, repr, &leaf, &x, sib, side, 3, nullptr) == ZK_EINVAL);
  EXPECT(zk_merkle_verify_proof((zk_field)3, repr, &leaf, &x, sib, side, 3, &ok) == ZK_EINVAL);
  EXPECT(ok == -5);  // nothing written by a failing call
  // random proofs of random lengths just fold
  for (int rep = 0; rep < 50; ++rep) {
    const size_t len = rnd() % 40;
    std::vector<zk_fe> s(len + 1);
    std::vector<uint8_t> sd(len + 1);
    for (size_t i = 0; i < len; ++i) {
      s[i] = small_fe();
      sd[i] = (uint8_t)(rnd() & 1);
    }
    EXPECT(zk_merkle_verify_proof(field, repr, &leaf, &x, s.data(), sd.data(), len, &ok) == ZK_OK && (ok == 0 || len == 0));
  }
}

// without a device there is no context, hence no tree: every tree call fails cleanly
static void no_device() {
  zk_ctx* ctx = nullptr;
  EXPECT(zk_ctx_create(0, &ctx) == ZK_EDEVICE && ctx == nullptr);
  zk_merkle* tree = nullptr;
  const zk_fe in[2] = {small_fe(), small_fe()};
  EXPECT(zk_merkle_new(ctx, ZK_BN254_FQ, 3, ZK_REPR_CANONICAL, in, 2, &tree) == ZK_EINVAL && tree == nullptr);
  EXPECT(zk_merkle_new(ctx, ZK_BN254_FQ, 0, ZK_REPR_CANONICAL, nullptr, 0, &tree) == ZK_EINVAL && tree == nullptr);
  EXPECT(zk_merkle_new(ctx, ZK_BN254_FQ, 3, ZK_REPR_CANONICAL, in, 2, nullptr) == ZK_EINVAL);
  EXPECT(zk_dev_merkle_new(ctx, ZK_BN254_FQ, 3, nullptr, 0, &tree) == ZK_EINVAL && tree == nullptr);
  EXPECT(zk_last_error()[0] != '\0');
  zk_fe out = in[0];
  uint64_t id = 0;
  uint8_t flag = 0, side = 7;
  EXPECT(zk_merkle_root(nullptr, ZK_REPR_CANONICAL, &out) == ZK_EINVAL);
  EXPECT(zk_merkle_download(nullptr, 0, ZK_REPR_CANONICAL, &out) == ZK_EINVAL);
  EXPECT(zk_merkle_update_leaves(nullptr, ZK_REPR_CANONICAL, &id, in, &flag, 1) == ZK_EINVAL);
  EXPECT(zk_merkle_create_proofs(nullptr, ZK_REPR_CANONICAL, in, &id, 1, &out, &side) == ZK_EINVAL);
  EXPECT(same(out, in[0]) && side == 7);
  zk_merkle_free(nullptr);
}

int main() {
  for (int field = 0; field < 3; ++field)
    for (int repr = 0; repr < 2; ++repr) {
      for (unsigned depth : {1u, 2u, 5u}) valid_proofs((zk_field)field, (zk_repr)repr, depth);
      hostile_inputs((zk_field)field, (zk_repr)repr);
    }
  no_device();
  if (failures) {
    fprintf(stderr, "merkle_asan_check: %d failure(s)\n", failures);
    return 1;
  }
  printf("merkle_asan_check ok\n");
  return 0;
}
