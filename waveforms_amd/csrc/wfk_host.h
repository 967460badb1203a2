// wfk_host.h -- what the host side of every stage shares: the error helper, the element kind and its size, the launch
// arithmetic of the row-slot kernels, the row rule of the one-size stages (the rule itself: wfk_row_rule.h), the
// device probe, the owners of a plan's device memory (DevBuf, MappedWord), the packer of several host tables into one
// device block (DevTables), next to the prototypes of the functions one stage's file calls in another's
// (wfk_internal.h).  Host code only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "wfk.h"
#include "wfk_internal.h"
#include "wfk_row_rule.h"

namespace {

inline int wfk_fail(int code, const std::string& m) {
  wfk_internal_set_error(m.c_str());
  return code;
}

// bytes of one real sample of a plan's kind
inline size_t wfk_elem_size(int kind) { return kind == WFK_OUT_F32 ? 4 : 8; }

// the kinds a stage takes; `who` ("", "IIR ", ...) goes in front of the text
inline int wfk_check_kind(int kind, const char* who = "") {
  if (kind == WFK_OUT_F64 || kind == WFK_OUT_F32) return WFK_OK;
  return wfk_fail(WFK_EINVAL, std::string(who) + "kind must be F64 or F32");
}

// Workgroups per row of a row-slot kernel (wfk_rows_dev.h): ceil((n + lead) / per_block) for rows of n >= 0 elements,
// a workgroup covering per_block of them.  `lead`: the elements a row may start into its first slot, V - 1 where the
// slots are laid out from a 16-byte boundary, 0 where they start at the row.  The grid is flat, batch >= 1 rows times
// these blocks in x: more than 2^31 - 1 is refused.  (Written so that no n overflows.)
inline int wfk_row_blocks(const char* stage, int64_t n, int64_t per_block, int64_t lead, int64_t batch,
                          uint32_t* blocks_per_row) {
  const int64_t bpr = n ? (n - 1) / per_block + ((n - 1) % per_block + lead) / per_block + 1 : 0;
  if (bpr > 0x7fffffffLL / batch) return wfk_fail(WFK_EINVAL, std::string(stage) + ": batch * n too large for one launch");
  *blocks_per_row = (uint32_t)bpr;
  return WFK_OK;
}

// The row rule (wfk_row_rule.h; DESIGN.md "The row rule") of the stages whose two sides have one row length and one
// element size, alignment left to the caller:
// `in` (in_rows rows) and `out` (out_rows rows) are there, no row stride is below n and -- `disjoint`, the
// out-of-place stages -- the two extents do not meet.  A stage whose rows all read ONE input row gives in_rows = 1; a
// launch without an input gives `out` twice.
inline int wfk_check_rows(const char* stage, int64_t n, size_t es, const void* in, int64_t in_rows, int64_t in_stride,
                          const void* out, int64_t out_rows, int64_t out_stride, bool disjoint = false) {
  return wfk_row_rule(stage, {{"in", in, in_rows, in_stride, n, es}}, {"out", out, out_rows, out_stride, n, es},
                      disjoint ? kRowsDisjoint : 0u, wfk_fail);
}

// A counting stage's report, zeroed on the stream before the kernel adds to it: an apply overwrites its report.  The
// n == 0 exit of such a stage is this alone, so it holds the report to its alignment itself.
inline int wfk_zero_report(const char* stage, const RowReport& report, hipStream_t s) {
  if (const int rc = wfk_report_rule(stage, report, wfk_fail)) return rc;
  if (!report.ptr || wfk_internal_zero_async(const_cast<void*>(report.ptr), report.bytes(), s) == WFK_OK) return WFK_OK;
  return wfk_fail(WFK_EHIP, std::string(stage) + ": zeroing the counts failed");
}

inline bool wfk_have_device() {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0) return true;
  (void)hipGetLastError();
  return false;
}

// owner of one device allocation
template <typename T>
class DevBuf {
  T* p_ = nullptr;

 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
  DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p_, o.p_); return *this; }
  ~DevBuf() { if (p_) (void)hipFree(p_); }
  bool alloc(size_t bytes) { return hipMalloc((void**)&p_, bytes) == hipSuccess; }
  bool upload(const void* src, size_t bytes) {
    return alloc(bytes) && hipMemcpy(p_, src, bytes, hipMemcpyHostToDevice) == hipSuccess;
  }
  bool upload(const std::vector<T>& src) { return upload(src.data(), src.size() * sizeof(T)); }
  T* get() const { return p_; }
  explicit operator bool() const { return p_ != nullptr; }
};

// owner of one word of mapped host memory that kernels raise and the host polls (a plan's fault word)
class MappedWord {
  unsigned* host_ = nullptr;
  unsigned* dev_ = nullptr;

 public:
  MappedWord() = default;
  MappedWord(const MappedWord&) = delete;
  MappedWord& operator=(const MappedWord&) = delete;
  ~MappedWord() { if (host_) (void)hipHostFree(host_); }
  bool alloc() {
    if (hipHostMalloc((void**)&host_, 64, hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer((void**)&dev_, host_, 0) != hipSuccess)
      return false;
    *host_ = 0;
    return true;
  }
  volatile unsigned* host() const { return host_; }
  unsigned* dev() const { return dev_; }
};

// Several host tables packed into ONE device block, each at a 256-byte boundary: add() copies a table into the
// host image and returns its offset, reserve() leaves room for a region the caller uploads on its own (a time axis
// as large as the output), total() is the size of the block to take (a spare 256 bytes behind the last table),
// upload() sends the image in one copy, at<T>() is the typed address of an offset in the block.  reserve() comes
// after the last add(): the image ends where the first reserved region starts.
class DevTables {
  std::vector<char> image_;   // [0, offset of the first reserved region)
  size_t end_ = 0;

  static size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

 public:
  size_t add(const void* src, size_t bytes) {
    const size_t o = reserve(bytes);
    image_.resize(end_, 0);
    if (bytes) std::memcpy(image_.data() + o, src, bytes);
    return o;
  }
  template <typename T>
  size_t add(const std::vector<T>& v) { return add(v.data(), v.size() * sizeof(T)); }
  size_t reserve(size_t bytes) {
    const size_t o = end_;
    end_ = align256(o + bytes);
    return o;
  }
  size_t total() const { return end_ + 256; }
  const std::vector<char>& image() const { return image_; }
  bool upload(void* block) const {
    return image_.empty() || hipMemcpy(block, image_.data(), image_.size(), hipMemcpyHostToDevice) == hipSuccess;
  }
  template <typename T>
  static T* at(void* block, size_t offset) { return reinterpret_cast<T*>(static_cast<char*>(block) + offset); }
};

// a plan's tables: the block taken and the image sent to it; `plan` ("dac rows plan") names the failure
inline int wfk_upload_tables(const char* plan, const DevTables& tab, DevBuf<char>& block) {
  if (block.alloc(tab.total()) && tab.upload(block.get())) return WFK_OK;
  (void)hipGetLastError();
  return wfk_fail(WFK_EHIP, std::string(plan) + ": table upload failed");
}

}  // namespace
