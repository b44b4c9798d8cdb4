// runtime_vocab.cpp -- the orb_vocabulary and orb_kf_database handles: DBoW2
// transform and scoring, and place recognition over the keyframe database.
#include "runtime_common.h"

extern "C" {

// ------------------------------------------------------- DBoW2 vocabulary
// (struct orb_vocabulary: runtime_common.h)
static orb_status_t vocab_build(orb_vocabulary* V, int n_nodes, const int32_t* parent,
                                const uint8_t* leaf, const uint8_t* desc, const double* weight) {
  // children in creation order (m_nodes[pid].children.push_back(nid), :1416)
  std::vector<int32_t> ccount(n_nodes, 0), cstart(n_nodes + 1, 0), clist(std::max(n_nodes - 1, 1));
  for (int i = 1; i < n_nodes; ++i) {
    if (parent[i] < 0 || parent[i] >= i) return ORB_EINVAL;
    ++ccount[parent[i]];
  }
  for (int i = 0; i < n_nodes; ++i) cstart[i + 1] = cstart[i] + ccount[i];
  {
    std::vector<int32_t> fill(cstart.begin(), cstart.end() - 1);
    for (int i = 1; i < n_nodes; ++i) clist[fill[parent[i]]++] = i;
  }
  // word ids: leaf-flagged nodes in file order (:1432-1439); others keep 0 (Node())
  std::vector<uint32_t> wordOf(n_nodes, 0);
  int nw = 0;
  for (int i = 1; i < n_nodes; ++i)
    if (leaf[i]) wordOf[i] = (uint32_t)nw++;
  // breadth-first renumbering: children of the node at position p occupy
  // consecutive positions, in child order
  std::vector<VocNodeInfo> info(n_nodes);
  std::vector<int32_t> orig(n_nodes);
  std::vector<uint8_t> ddesc((size_t)n_nodes * 32);
  std::vector<uint32_t> dword(n_nodes);
  std::vector<double> dweight(n_nodes);
  orig[0] = 0;
  int next = 1;
  for (int p = 0; p < n_nodes; ++p) {
    const int id = orig[p];
    info[p].first = next;
    info[p].count = ccount[id];
    for (int c = cstart[id]; c < cstart[id + 1]; ++c) orig[next++] = clist[c];
    memcpy(&ddesc[(size_t)p * 32], desc + (size_t)id * 32, 32);
    dword[p] = wordOf[id];
    dweight[p] = id == 0 ? 0.0 : weight[id];
  }
  if (next != n_nodes) return ORB_EINVAL;
  V->nNodes = n_nodes;
  V->nWords = nw;
  hipStream_t s = V->stream;
  orb_status_t st;
  if ((st = upload(V->dInfo, info.data(), info.size() * sizeof(VocNodeInfo), s))) return st;
  if ((st = upload(V->dDesc, ddesc.data(), ddesc.size(), s))) return st;
  if ((st = upload(V->dWord, dword.data(), dword.size() * 4, s))) return st;
  if ((st = upload(V->dWeight, dweight.data(), dweight.size() * 8, s))) return st;
  if ((st = upload(V->dOrig, orig.data(), orig.size() * 4, s))) return st;
  HIP_TRY(stream_wait(s));
  return ORB_OK;
}

static orb_status_t vocab_new(int device, int k, int L, int scoring, int weighting,
                              orb_vocabulary** out) {
  orb_status_t st = check_device(device);
  if (st) return st;
  orb_vocabulary* V = new orb_vocabulary();
  V->device = device;
  V->k = k; V->L = L; V->scoring = scoring; V->weighting = weighting;
  hipSetDevice(device);
  if (create_own_stream(&V->stream) != hipSuccess) {
    delete V;
    return ORB_EDEVICE;
  }
  *out = V;
  return ORB_OK;
}

orb_status_t orb_vocabulary_create(int device, int k, int L, int scoring, int weighting,
                                   int n_nodes, const int32_t* parent, const uint8_t* leaf_flag,
                                   const uint8_t* descriptors, const double* weights,
                                   orb_vocabulary_t** out) {
  if (!out) return ORB_EINVAL;
  *out = nullptr;
  // loadFromTextFile's header check (:1383)
  if (k < 0 || k > 20 || L < 1 || L > 10 || scoring < 0 || scoring > 5 || weighting < 0 ||
      weighting > 3 || n_nodes < 1 ||
      (n_nodes > 1 && (!parent || !leaf_flag || !descriptors || !weights)))
    return ORB_EINVAL;
  orb_vocabulary* V = nullptr;
  orb_status_t st = vocab_new(device, k, L, scoring, weighting, &V);
  if (st) return st;
  std::vector<int32_t> p0(1, 0);
  std::vector<uint8_t> l0(1, 0), d0(32, 0);
  std::vector<double> w0(1, 0.0);
  st = n_nodes > 1 ? vocab_build(V, n_nodes, parent, leaf_flag, descriptors, weights)
                   : vocab_build(V, 1, p0.data(), l0.data(), d0.data(), w0.data());
  if (st) {
    orb_vocabulary_destroy(V);
    return st;
  }
  *out = V;
  return ORB_OK;
}

// Text format of loadFromTextFile: "k L scoring weighting", then one line per
// node "parent isLeaf d0 .. d31 weight" (descriptor bytes as integers,
// FORB::fromString FORB.cpp:120-135).  Lines without a parent field are
// skipped (the reference's eof loop turns a trailing empty line into a root
// child with an uninitialised descriptor).
orb_status_t orb_vocabulary_load_text(int device, const char* path, orb_vocabulary_t** out) {
  if (!out || !path) return ORB_EINVAL;
  *out = nullptr;
  FILE* fp = fopen(path, "rb");
  if (!fp) return ORB_EINVAL;
  std::vector<char> text;
  {
    char buf[1 << 16];
    size_t r;
    while ((r = fread(buf, 1, sizeof(buf), fp)) > 0) text.insert(text.end(), buf, buf + r);
    fclose(fp);
  }
  text.push_back('\0');
  char* c = text.data();
  char* eol = strchr(c, '\n');
  int hdr[4];
  for (int i = 0; i < 4; ++i) {
    char* e;
    const long v = strtol(c, &e, 10);
    if (e == c || (eol && e > eol)) return ORB_EINVAL;
    hdr[i] = (int)v;
    c = e;
  }
  c = eol ? eol + 1 : c + strlen(c);
  std::vector<int32_t> parent(1, 0);
  std::vector<uint8_t> leaf(1, 0), desc(32, 0);
  std::vector<double> weight(1, 0.0);
  while (*c) {
    char* le = strchr(c, '\n');
    if (le) *le = '\0';
    char* e;
    const long pid = strtol(c, &e, 10);
    if (e != c) {
      c = e;
      const long isLeaf = strtol(c, &e, 10);
      c = e;
      uint8_t d[32] = {0};
      for (int i = 0; i < 32; ++i) {
        const long v = strtol(c, &e, 10);
        if (e == c) break;
        d[i] = (uint8_t)v;
        c = e;
      }
      const double w = strtod(c, &e);
      parent.push_back((int32_t)pid);
      leaf.push_back(isLeaf > 0);
      desc.insert(desc.end(), d, d + 32);
      weight.push_back(e == c ? 0.0 : w);
    }
    if (!le) break;
    c = le + 1;
  }
  return orb_vocabulary_create(device, hdr[0], hdr[1], hdr[2], hdr[3], (int)parent.size(),
                               parent.data(), leaf.data(), desc.data(), weight.data(), out);
}

void orb_vocabulary_destroy(orb_vocabulary_t* V) {
  if (!V) return;
  hipSetDevice(V->device);
  hipStreamSynchronize(V->stream);
  const hipStream_t stream = V->stream;
  delete V;  // frees every buffer (DevBuf)
  hipStreamDestroy(stream);
}

orb_status_t orb_vocabulary_info(const orb_vocabulary_t* V, int32_t* info6) {
  if (!V || !info6) return ORB_EINVAL;
  info6[0] = V->k; info6[1] = V->L; info6[2] = V->scoring; info6[3] = V->weighting;
  info6[4] = V->nNodes; info6[5] = V->nWords;
  return ORB_OK;
}

void* orb_vocabulary_stream(orb_vocabulary_t* V) { return V ? (void*)V->stream : nullptr; }

static orb_status_t vocab_launch(orb_vocabulary* V, int n_frames, const int32_t* d_counts,
                                 int n_single, const uint8_t* d_desc, int stride, int levelsup,
                                 uint32_t* fword, double* fweight, uint32_t* fnode,
                                 uint32_t* bw, double* bv, int32_t* nw, uint32_t* fvn,
                                 int32_t* fvo, uint32_t* fvf, int32_t* nfv, hipStream_t s) {
  int l2 = V->scoring == 1;
  const int must = V->scoring != 5;  // ScoringObject.h:74-89
  const int tf = V->weighting == 0 || V->weighting == 1;
  if (V->nWords == 0) {  // empty(): v, fv cleared (:1136-1140)
    HIP_TRY(hipMemsetAsync(nw, 0, (size_t)n_frames * 4, s));
    HIP_TRY(hipMemsetAsync(nfv, 0, (size_t)n_frames * 4, s));
    for (int f = 0; f < n_frames; ++f)
      HIP_TRY(hipMemsetAsync(fvo + (size_t)f * (stride + 1), 0, 4, s));
    return ORB_OK;
  }
  HIP_TRY(orb_k_voc_descend(V->dInfo.as<VocNodeInfo>(), V->dDesc.p, V->dWord.as<uint32_t>(),
                            V->dWeight.as<double>(), V->dOrig.as<uint32_t>(), V->L - levelsup,
                            d_desc, d_counts, n_single, stride, n_frames, fword, fweight, fnode,
                            s));
  HIP_TRY(orb_k_voc_vectors(fword, fweight, fnode, d_counts, n_single, stride, tf, must, l2,
                            n_frames, bw, bv, nw, fvn, fvo, fvf, nfv, s));
  return ORB_OK;
}

orb_status_t orb_vocabulary_transform(orb_vocabulary_t* V, int n, const uint8_t* desc,
                                      int levelsup, uint32_t* bow_words, double* bow_values,
                                      int32_t* n_words, uint32_t* fv_nodes, int32_t* fv_offs,
                                      uint32_t* fv_feats, int32_t* n_fv_nodes,
                                      uint32_t* feat_word, uint32_t* feat_node) {
  if (!V || n < 0 || n > orb_k_voc_max_features() || (n > 0 && !desc) || !bow_words ||
      !bow_values || !n_words || !fv_nodes || !fv_offs || !fv_feats || !n_fv_nodes)
    return ORB_EINVAL;
  if (n == 0 || V->nWords == 0) {
    *n_words = 0;
    *n_fv_nodes = 0;
    fv_offs[0] = 0;
    return ORB_OK;
  }
  std::lock_guard<std::mutex> g(V->mu);
  hipSetDevice(V->device);
  hipStream_t s = V->stream;
  orb_status_t st;
  const size_t N = (size_t)n;
  if ((st = upload(V->dIn, desc, N * 32, s))) return st;
  if ((st = V->dFWord.ensure(N * 4)) || (st = V->dFWeight.ensure(N * 8)) ||
      (st = V->dFNode.ensure(N * 4)) || (st = V->dBowW.ensure(N * 4)) ||
      (st = V->dBowV.ensure(N * 8)) || (st = V->dNW.ensure(16)) || (st = V->dFvN.ensure(N * 4)) ||
      (st = V->dFvO.ensure((N + 1) * 4)) || (st = V->dFvF.ensure(N * 4)) ||
      (st = V->dNFv.ensure(16)))
    return st;
  if ((st = vocab_launch(V, 1, nullptr, n, V->dIn.as<uint8_t>(), n, levelsup,
                         V->dFWord.as<uint32_t>(), V->dFWeight.as<double>(),
                         V->dFNode.as<uint32_t>(), V->dBowW.as<uint32_t>(),
                         V->dBowV.as<double>(), V->dNW.as<int32_t>(), V->dFvN.as<uint32_t>(),
                         V->dFvO.as<int32_t>(), V->dFvF.as<uint32_t>(), V->dNFv.as<int32_t>(), s)))
    return st;
  int32_t counts[2];
  HIP_TRY(hipMemcpyAsync(&counts[0], V->dNW.p, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&counts[1], V->dNFv.p, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(stream_wait(s));
  *n_words = counts[0];
  *n_fv_nodes = counts[1];
  HIP_TRY(hipMemcpyAsync(bow_words, V->dBowW.p, (size_t)counts[0] * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(bow_values, V->dBowV.p, (size_t)counts[0] * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(fv_nodes, V->dFvN.p, (size_t)counts[1] * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(fv_offs, V->dFvO.p, (size_t)(counts[1] + 1) * 4, hipMemcpyDeviceToHost,
                         s));
  HIP_TRY(stream_wait(s));
  const int nfeat = fv_offs[counts[1]];
  if (nfeat > 0)
    HIP_TRY(hipMemcpyAsync(fv_feats, V->dFvF.p, (size_t)nfeat * 4, hipMemcpyDeviceToHost, s));
  if (feat_word) HIP_TRY(hipMemcpyAsync(feat_word, V->dFWord.p, N * 4, hipMemcpyDeviceToHost, s));
  if (feat_node) HIP_TRY(hipMemcpyAsync(feat_node, V->dFNode.p, N * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(stream_wait(s));
  return ORB_OK;
}

orb_status_t orb_vocabulary_transform_batch(orb_vocabulary_t* V, int n_frames,
                                            const int32_t* d_counts, const uint8_t* d_desc,
                                            int stride, int levelsup, uint32_t* d_feat_word,
                                            double* d_feat_weight, uint32_t* d_feat_node,
                                            uint32_t* d_bow_words, double* d_bow_values,
                                            int32_t* d_n_words, uint32_t* d_fv_nodes,
                                            int32_t* d_fv_offs, uint32_t* d_fv_feats,
                                            int32_t* d_n_fv_nodes, void* stream) {
  if (!V || n_frames < 0 || stride <= 0 || stride > orb_k_voc_max_features()) return ORB_EINVAL;
  if (n_frames == 0) return ORB_OK;
  if (!d_counts || !d_desc || !d_feat_word || !d_feat_weight || !d_feat_node || !d_bow_words ||
      !d_bow_values || !d_n_words || !d_fv_nodes || !d_fv_offs || !d_fv_feats || !d_n_fv_nodes)
    return ORB_EINVAL;
  hipSetDevice(V->device);
  return vocab_launch(V, n_frames, d_counts, 0, d_desc, stride, levelsup, d_feat_word,
                      d_feat_weight, d_feat_node, d_bow_words, d_bow_values, d_n_words,
                      d_fv_nodes, d_fv_offs, d_fv_feats, d_n_fv_nodes,
                      stream ? (hipStream_t)stream : V->stream);
}

// ------------------------------------------------- place recognition: score
// TemplatedVocabulary::score -> ScoringObject.cpp:23-311 (placerec_kernels.hip).
static bool bow_vectors_valid(int n, const int32_t* offs, const uint32_t* words) {
  if (offs[0] < 0) return false;
  for (int p = 0; p < n; ++p) {
    if (offs[p + 1] < offs[p]) return false;
    for (int i = offs[p] + 1; i < offs[p + 1]; ++i)
      if (words[i] <= words[i - 1]) return false;  // std::map keys: strictly ascending
  }
  return true;
}

orb_status_t orb_vocabulary_score(orb_vocabulary_t* V, int n_pairs, const int32_t* a_offs,
                                  const uint32_t* a_words, const double* a_values,
                                  const int32_t* b_offs, const uint32_t* b_words,
                                  const double* b_values, double* out) {
  if (!V || n_pairs < 0 || V->scoring == ORB_VOC_KL) return ORB_EINVAL;
  if (n_pairs == 0) return ORB_OK;
  if (!a_offs || !b_offs || !out) return ORB_EINVAL;
  const size_t na = (size_t)std::max(a_offs[n_pairs], 0), nb = (size_t)std::max(b_offs[n_pairs], 0);
  if ((na && (!a_words || !a_values)) || (nb && (!b_words || !b_values))) return ORB_EINVAL;
  if (!bow_vectors_valid(n_pairs, a_offs, a_words) || !bow_vectors_valid(n_pairs, b_offs, b_words))
    return ORB_EINVAL;
  std::lock_guard<std::mutex> g(V->mu);
  hipSetDevice(V->device);
  hipStream_t s = V->stream;
  orb_status_t st;
  DevBuf* B = V->dScore;
  const size_t no = (size_t)(n_pairs + 1) * 4;
  if ((st = upload(B[0], a_offs, no, s)) || (st = upload(B[1], a_words, na * 4, s)) ||
      (st = upload(B[2], a_values, na * 8, s)) || (st = upload(B[3], b_offs, no, s)) ||
      (st = upload(B[4], b_words, nb * 4, s)) || (st = upload(B[5], b_values, nb * 8, s)) ||
      (st = B[6].ensure((size_t)n_pairs * 8)))
    return st;
  HIP_TRY(orb_k_bow_score(V->scoring, n_pairs, B[0].as<int32_t>(), B[1].as<uint32_t>(),
                          B[2].as<double>(), B[3].as<int32_t>(), B[4].as<uint32_t>(),
                          B[5].as<double>(), B[6].as<double>(), s));
  HIP_TRY(hipMemcpyAsync(out, B[6].p, (size_t)n_pairs * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(stream_wait(s));
  return ORB_OK;
}

orb_status_t orb_vocabulary_score_batch(orb_vocabulary_t* V, int n_pairs, const int32_t* d_a_offs,
                                        const uint32_t* d_a_words, const double* d_a_values,
                                        const int32_t* d_b_offs, const uint32_t* d_b_words,
                                        const double* d_b_values, double* d_out, void* stream) {
  if (!V || n_pairs < 0 || V->scoring == ORB_VOC_KL) return ORB_EINVAL;
  if (n_pairs == 0) return ORB_OK;
  if (!d_a_offs || !d_a_words || !d_a_values || !d_b_offs || !d_b_words || !d_b_values || !d_out)
    return ORB_EINVAL;
  hipSetDevice(V->device);
  HIP_TRY(orb_k_bow_score(V->scoring, n_pairs, d_a_offs, d_a_words, d_a_values, d_b_offs,
                          d_b_words, d_b_values, d_out, stream ? (hipStream_t)stream : V->stream));
  return ORB_OK;
}

// -------------------------------------- place recognition: KeyFrameDatabase
// src/KeyFrameDatabase.cc over keyframe ids.  A keyframe takes the next slot
// when it is added; slots are never reused before clear(), so the slot index
// is the add sequence number the list order needs (placerec_kernels.hip).
// The host keeps what resolves ids (id -> slot, who names whom as a
// neighbour); BowVectors, covisibility slots and scores stay on the device.
struct orb_kf_database {
  orb_vocabulary* voc = nullptr;
  int device = 0;
  hipStream_t stream = nullptr;
  std::mutex mu;
  // host side of the slot table
  std::vector<int64_t> slotId;
  std::vector<uint8_t> slotLive;
  std::vector<std::array<int64_t, PR_NEIGH>> neighIds;
  std::vector<int> neighN;
  std::unordered_map<int64_t, int> slotOf;  // live keyframes
  // neighbour id -> (slot, position) of every live keyframe that names it
  std::unordered_multimap<int64_t, std::pair<int, int>> namedBy;
  size_t entries = 0;  // BowVector entries stored (erased ones included)
  int nLive = 0;
  // device: the database (grown with their contents kept)
  DevBuf dWords, dValues, dSlots, dNeigh, dIds, dStored[2];  // [0] mRelocScore, [1] mLoopScore
  // device: per-query scratch
  DevBuf dQW, dQV, dConnSlots, dConn, dCommon, dFirst, dFirstPos, dKeys, dList, dHdr, dScored,
      dAcc, dBest, dValid, dOut;
  uint64_t lastId[2] = {0, 0};
  int lastKind = -1, lastSlots = 0, lastN = 0;
  bool argsValid = false;
  PrQueryArgs args;
};

// Grows b to hold `need` bytes, keeping its first `used` bytes.
static orb_status_t grow_keep(DevBuf& b, size_t used, size_t need, hipStream_t s) {
  if (need <= b.bytes) return ORB_OK;
  const size_t cap = std::max<size_t>(std::max(need, b.bytes * 2), 4096);
  void* p = nullptr;
  if (hipMalloc(&p, cap) != hipSuccess) return ORB_ENOMEM;
  if (used && b.p) {
    hipError_t e = hipMemcpyAsync(p, b.p, used, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
      hipFree(p);
      return ORB_EDEVICE;
    }
  }
  if (b.p) hipFree(b.p);
  b.p = p;
  b.bytes = cap;
  return ORB_OK;
}

static void kfdb_unname(orb_kf_database* D, int slot) {
  for (int j = 0; j < D->neighN[slot]; ++j) {
    auto range = D->namedBy.equal_range(D->neighIds[slot][j]);
    for (auto it = range.first; it != range.second; ++it)
      if (it->second.first == slot && it->second.second == j) {
        D->namedBy.erase(it);
        break;
      }
  }
  D->neighN[slot] = 0;
}

// Every live keyframe that names `id` as a neighbour now points at `slot` (-1: absent).
static orb_status_t kfdb_patch_neighbours(orb_kf_database* D, int64_t id, const int32_t* slot,
                                          hipStream_t s) {
  auto range = D->namedBy.equal_range(id);
  for (auto it = range.first; it != range.second; ++it) {
    const size_t at = (size_t)it->second.first * PR_NEIGH + it->second.second;
    HIP_TRY(hipMemcpyAsync(D->dNeigh.as<int32_t>() + at, slot, 4, hipMemcpyHostToDevice, s));
  }
  return ORB_OK;
}

orb_status_t orb_kf_database_create(orb_vocabulary_t* V, orb_kf_database_t** out) {
  if (!out) return ORB_EINVAL;
  *out = nullptr;
  if (!V || V->scoring == ORB_VOC_KL) return ORB_EINVAL;
  orb_kf_database* D = new orb_kf_database();
  D->voc = V;
  D->device = V->device;
  hipSetDevice(D->device);
  if (create_own_stream(&D->stream) != hipSuccess) {
    delete D;
    return ORB_EDEVICE;
  }
  *out = D;
  return ORB_OK;
}

void orb_kf_database_destroy(orb_kf_database_t* D) {
  if (!D) return;
  hipSetDevice(D->device);
  hipStreamSynchronize(D->stream);
  const hipStream_t stream = D->stream;
  delete D;  // frees every buffer (DevBuf)
  hipStreamDestroy(stream);
}

orb_status_t orb_kf_database_clear(orb_kf_database_t* D) {
  if (!D) return ORB_EINVAL;
  std::lock_guard<std::mutex> g(D->mu);
  D->slotId.clear();
  D->slotLive.clear();
  D->neighIds.clear();
  D->neighN.clear();
  D->slotOf.clear();
  D->namedBy.clear();
  D->entries = 0;
  D->nLive = 0;
  D->lastKind = -1;
  D->lastN = D->lastSlots = 0;
  D->argsValid = false;
  return ORB_OK;
}

int orb_kf_database_size(orb_kf_database_t* D) {
  if (!D) return ORB_EINVAL;
  std::lock_guard<std::mutex> g(D->mu);
  return D->nLive;
}

orb_status_t orb_kf_database_add(orb_kf_database_t* D, int64_t kf_id, int n_words,
                                 const uint32_t* words, const double* values) {
  if (!D || n_words < 0 || (n_words > 0 && (!words || !values))) return ORB_EINVAL;
  for (int i = 0; i < n_words; ++i)
    if (words[i] >= (uint32_t)D->voc->nWords || (i > 0 && words[i] <= words[i - 1]))
      return ORB_EINVAL;
  std::lock_guard<std::mutex> g(D->mu);
  if (D->slotOf.count(kf_id) || D->slotId.size() >= (size_t)0x7FFFFFFF) return ORB_EINVAL;
  hipSetDevice(D->device);
  hipStream_t s = D->stream;
  const size_t slot = D->slotId.size(), e0 = D->entries, e1 = e0 + (size_t)n_words;
  orb_status_t st;
  if ((st = grow_keep(D->dWords, e0 * 4, e1 * 4, s)) ||
      (st = grow_keep(D->dValues, e0 * 8, e1 * 8, s)) ||
      (st = grow_keep(D->dSlots, slot * sizeof(PrSlot), (slot + 1) * sizeof(PrSlot), s)) ||
      (st = grow_keep(D->dNeigh, slot * PR_NEIGH * 4, (slot + 1) * PR_NEIGH * 4, s)) ||
      (st = grow_keep(D->dIds, slot * 8, (slot + 1) * 8, s)) ||
      (st = grow_keep(D->dStored[0], slot * 4, (slot + 1) * 4, s)) ||
      (st = grow_keep(D->dStored[1], slot * 4, (slot + 1) * 4, s)))
    return st;
  const PrSlot rec{(long long)e0, n_words, 1};
  int32_t none[PR_NEIGH];
  for (int32_t& v : none) v = -1;
  const long long id = kf_id;
  const int32_t self = (int32_t)slot;
  if (n_words) {
    HIP_TRY(hipMemcpyAsync(D->dWords.as<uint32_t>() + e0, words, (size_t)n_words * 4,
                           hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(D->dValues.as<double>() + e0, values, (size_t)n_words * 8,
                           hipMemcpyHostToDevice, s));
  }
  HIP_TRY(hipMemcpyAsync(D->dSlots.as<PrSlot>() + slot, &rec, sizeof(rec),
                         hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(D->dNeigh.as<int32_t>() + slot * PR_NEIGH, none, sizeof(none),
                         hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(D->dIds.as<long long>() + slot, &id, 8, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemsetAsync(D->dStored[0].as<float>() + slot, 0, 4, s));  // never scored: 0.0f
  HIP_TRY(hipMemsetAsync(D->dStored[1].as<float>() + slot, 0, 4, s));
  if ((st = kfdb_patch_neighbours(D, kf_id, &self, s))) return st;
  HIP_TRY(hipStreamSynchronize(s));
  D->slotId.push_back(kf_id);
  D->slotLive.push_back(1);
  D->neighIds.emplace_back();
  D->neighN.push_back(0);
  D->slotOf[kf_id] = (int)slot;
  D->entries = e1;
  ++D->nLive;
  D->argsValid = false;
  return ORB_OK;
}

orb_status_t orb_kf_database_erase(orb_kf_database_t* D, int64_t kf_id) {
  if (!D) return ORB_EINVAL;
  std::lock_guard<std::mutex> g(D->mu);
  auto it = D->slotOf.find(kf_id);
  if (it == D->slotOf.end()) return ORB_OK;
  hipSetDevice(D->device);
  hipStream_t s = D->stream;
  const int slot = it->second;
  const int32_t dead = 0, none = -1;
  HIP_TRY(hipMemcpyAsync(&D->dSlots.as<PrSlot>()[slot].live, &dead, 4, hipMemcpyHostToDevice,
                         s));
  orb_status_t st = kfdb_patch_neighbours(D, kf_id, &none, s);
  if (st) return st;
  HIP_TRY(hipStreamSynchronize(s));
  kfdb_unname(D, slot);
  D->slotLive[slot] = 0;
  D->slotOf.erase(it);
  --D->nLive;
  D->argsValid = false;
  return ORB_OK;
}

orb_status_t orb_kf_database_set_covisibility(orb_kf_database_t* D, int64_t kf_id, int n,
                                              const int64_t* neighbour_ids) {
  if (!D || n < 0 || n > PR_NEIGH || (n > 0 && !neighbour_ids)) return ORB_EINVAL;
  std::lock_guard<std::mutex> g(D->mu);
  auto it = D->slotOf.find(kf_id);
  if (it == D->slotOf.end()) return ORB_EINVAL;
  hipSetDevice(D->device);
  hipStream_t s = D->stream;
  const int slot = it->second;
  int32_t resolved[PR_NEIGH];
  for (int j = 0; j < PR_NEIGH; ++j) {
    resolved[j] = -1;
    if (j < n) {
      auto f = D->slotOf.find(neighbour_ids[j]);
      if (f != D->slotOf.end()) resolved[j] = f->second;
    }
  }
  HIP_TRY(hipMemcpyAsync(D->dNeigh.as<int32_t>() + (size_t)slot * PR_NEIGH, resolved,
                         sizeof(resolved), hipMemcpyHostToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));
  kfdb_unname(D, slot);
  for (int j = 0; j < n; ++j) {
    D->neighIds[slot][j] = neighbour_ids[j];
    D->namedBy.emplace(neighbour_ids[j], std::make_pair(slot, j));
  }
  D->neighN[slot] = n;
  D->argsValid = false;
  return ORB_OK;
}

static orb_status_t kfdb_query(orb_kf_database* D, int kind, uint64_t query_id, int n_words,
                               const uint32_t* words, const double* values, int n_connected,
                               const int64_t* connected_ids, float min_score, int64_t* out_ids,
                               int capacity, int* n_out) {
  if (!D || !n_out || n_words < 0 || (n_words > 0 && (!words || !values)) || capacity < 0 ||
      (capacity > 0 && !out_ids) || n_connected < 0 || (n_connected > 0 && !connected_ids))
    return ORB_EINVAL;
  for (int i = 0; i < n_words; ++i)
    if (words[i] >= (uint32_t)D->voc->nWords || (i > 0 && words[i] <= words[i - 1]))
      return ORB_EINVAL;
  std::lock_guard<std::mutex> g(D->mu);
  // mnRelocQuery / mnLoopQuery start at 0 and ids are unique in the reference
  if (query_id == 0 || query_id == D->lastId[kind]) return ORB_EINVAL;
  D->lastId[kind] = query_id;
  D->lastKind = kind;
  D->lastN = 0;
  D->argsValid = false;
  *n_out = 0;
  const int nSlots = (int)D->slotId.size();
  D->lastSlots = nSlots;
  if (nSlots == 0 || n_words == 0) return ORB_OK;  // nothing shares a word (:111, :238)
  hipSetDevice(D->device);
  hipStream_t s = D->stream;
  std::vector<int32_t> conn;
  for (int i = 0; i < n_connected; ++i) {
    auto f = D->slotOf.find(connected_ids[i]);
    if (f != D->slotOf.end()) conn.push_back(f->second);
  }
  const size_t N = (size_t)nSlots;
  orb_status_t st;
  if ((st = upload(D->dQW, words, (size_t)n_words * 4, s)) ||
      (st = upload(D->dQV, values, (size_t)n_words * 8, s)) ||
      (st = upload(D->dConnSlots, conn.data(), conn.size() * 4, s)) ||
      (st = D->dConn.ensure(N)) || (st = D->dCommon.ensure(N * 4)) ||
      (st = D->dFirst.ensure(N * 4)) || (st = D->dFirstPos.ensure(N * 4)) ||
      (st = D->dKeys.ensure(std::max<size_t>(orb_k_db_key_scratch(nSlots), 1) * 8)) ||
      (st = D->dList.ensure(N * 4)) || (st = D->dHdr.ensure(16)) || (st = D->dScored.ensure(N)) ||
      (st = D->dAcc.ensure(N * 4)) || (st = D->dBest.ensure(N * 4)) ||
      (st = D->dValid.ensure(N)) || (st = D->dOut.ensure(N * 8)))
    return st;
  PrQueryArgs& A = D->args;
  A.type = D->voc->scoring;
  A.loop = kind;
  A.minScore = min_score;
  A.nSlots = nSlots;
  A.nq = n_words;
  A.nConnected = (int)conn.size();
  A.slots = D->dSlots.as<PrSlot>();
  A.words = D->dWords.as<uint32_t>();
  A.values = D->dValues.as<double>();
  A.neigh = D->dNeigh.as<int32_t>();
  A.ids = D->dIds.as<long long>();
  A.stored = D->dStored[kind].as<float>();
  A.qWords = D->dQW.as<uint32_t>();
  A.qValues = D->dQV.as<double>();
  A.connSlots = D->dConnSlots.as<int32_t>();
  A.connected = D->dConn.as<uint8_t>();
  A.common = D->dCommon.as<int32_t>();
  A.first = D->dFirst.as<uint32_t>();
  A.firstPos = D->dFirstPos.as<int32_t>();
  A.keys = D->dKeys.as<unsigned long long>();
  A.list = D->dList.as<uint32_t>();
  A.hdr = D->dHdr.as<int32_t>();
  A.scored = D->dScored.as<uint8_t>();
  A.acc = D->dAcc.as<float>();
  A.best = D->dBest.as<uint32_t>();
  A.valid = D->dValid.as<uint8_t>();
  A.out = D->dOut.as<long long>();
  A.stage = -1;
  HIP_TRY(orb_k_db_query(&A, s));
  int32_t hdr[4];
  HIP_TRY(hipMemcpyAsync(hdr, D->dHdr.p, sizeof(hdr), hipMemcpyDeviceToHost, s));
  HIP_TRY(stream_wait(s));
  D->lastN = hdr[0];
  D->argsValid = true;
  *n_out = hdr[3];
  if (hdr[3] > capacity) return ORB_ECAPACITY;
  if (hdr[3] > 0) {
    HIP_TRY(hipMemcpyAsync(out_ids, D->dOut.p, (size_t)hdr[3] * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(stream_wait(s));
  }
  return ORB_OK;
}

orb_status_t orb_kf_database_detect_relocalization(orb_kf_database_t* D, uint64_t query_id,
                                                   int n_words, const uint32_t* words,
                                                   const double* values, int64_t* out_ids,
                                                   int capacity, int* n_out) {
  return kfdb_query(D, 0, query_id, n_words, words, values, 0, nullptr, 0.0f, out_ids, capacity,
                    n_out);
}

orb_status_t orb_kf_database_detect_loop(orb_kf_database_t* D, uint64_t query_id, int n_words,
                                         const uint32_t* words, const double* values,
                                         int n_connected, const int64_t* connected_ids,
                                         float min_score, int64_t* out_ids, int capacity,
                                         int* n_out) {
  return kfdb_query(D, 1, query_id, n_words, words, values, n_connected, connected_ids, min_score,
                    out_ids, capacity, n_out);
}

orb_status_t orb_kf_database_last_query(orb_kf_database_t* D, int64_t* ids, int32_t* common,
                                        float* scores, uint8_t* scored, int capacity, int* n) {
  if (!D || !n || capacity < 0) return ORB_EINVAL;
  std::lock_guard<std::mutex> g(D->mu);
  const int L = D->lastKind < 0 ? 0 : D->lastN;
  *n = L;
  if (L > capacity) return ORB_ECAPACITY;
  if (L == 0) return ORB_OK;
  hipSetDevice(D->device);
  hipStream_t s = D->stream;
  const size_t N = (size_t)D->lastSlots;
  std::vector<uint32_t> list(L);
  std::vector<int32_t> cm(N);
  std::vector<float> sc(N);
  HIP_TRY(hipMemcpyAsync(list.data(), D->dList.p, (size_t)L * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(cm.data(), D->dCommon.p, N * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(sc.data(), D->dStored[D->lastKind].p, N * 4, hipMemcpyDeviceToHost, s));
  if (scored) HIP_TRY(hipMemcpyAsync(scored, D->dScored.p, (size_t)L, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (int i = 0; i < L; ++i) {
    const uint32_t slot = list[i];
    if (slot >= N) return ORB_EDEVICE;
    if (ids) ids[i] = D->slotId[slot];
    if (common) common[i] = cm[slot];
    if (scores) scores[i] = sc[slot];
  }
  return ORB_OK;
}

orb_status_t orb_kf_database_profile(orb_kf_database_t* D, int stage, int reps, double* total_ms,
                                     const char** name) {
  static const char* const names[] = {"k_db_common", "k_db_list", "k_db_score", "k_db_accumulate",
                                      "k_db_select"};
  if (!D || stage < 0 || stage > 4 || reps < 1 || !total_ms) return ORB_EINVAL;
  std::lock_guard<std::mutex> g(D->mu);
  if (!D->argsValid) return ORB_EINVAL;
  hipSetDevice(D->device);
  hipStream_t s = D->stream;
  hipEvent_t e0, e1;
  HIP_TRY(hipEventCreate(&e0));
  HIP_TRY(hipEventCreate(&e1));
  PrQueryArgs A = D->args;
  A.stage = stage;
  hipError_t e = hipEventRecord(e0, s);
  for (int i = 0; i < reps && e == hipSuccess; ++i) e = orb_k_db_query(&A, s);
  if (e == hipSuccess) e = hipEventRecord(e1, s);
  if (e == hipSuccess) e = hipEventSynchronize(e1);
  float ms = 0.f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
  hipEventDestroy(e0);
  hipEventDestroy(e1);
  HIP_TRY(e);
  *total_ms = ms;
  if (name) *name = names[stage];
  return ORB_OK;
}

}  // extern "C"
