// owner_units.hip — the owning types of ws_internal.h (DevBuf, HostBlock, DevCounter) whichever way their allocation goes.  After
// WS_OK the pointer is there and the capacity is at least what was asked for; after an error the object is empty and the code is a
// WS_ERR_*; release() twice is safe either way, and a second attempt after a failure behaves like the first.  With a device every
// allocation succeeds; without one hipMalloc and hipHostMalloc fail (hipErrorNoDevice), which is the path no GPU test reaches.
#include <cstdint>
#include <cstdio>
#include <string>

#include "ws_internal.h"

using namespace ws;

static std::string g_error;
void ws::set_error(const std::string &msg) { g_error = msg; }
int ws::hip_fail(hipError_t e, const char *what, const char *, int)
{
  set_error(std::string(what) + ": " + hipGetErrorString(e));
  return WS_ERR_HIP;
}

static int g_ok = 0, g_failed = 0; // allocations that succeeded / failed

#define EXPECT(cond)                                             \
  do                                                             \
  {                                                              \
    if (!(cond))                                                 \
    {                                                            \
      printf("%s: %s (line %d)\n", what, #cond, __LINE__);       \
      return 1;                                                  \
    }                                                            \
  } while (0)

// the verdict on one attempt: `filled` / `empty` describe the object after it
static int verdict(const char *what, int rc, bool filled, bool empty)
{
  if (rc == WS_OK)
  {
    EXPECT(filled);
    ++g_ok;
  }
  else
  {
    EXPECT(rc < 0 && rc >= WS_ERR_INTERNAL); // a WS_ERR_*
    EXPECT(empty);
    EXPECT(!g_error.empty());
    ++g_failed;
  }
  return 0;
}

static int dev_buf(const char *what, bool by_alloc, DevBuf::Slack slack)
{
  const size_t need = 1000;
  DevBuf b;
  for (int attempt = 0; attempt < 2; ++attempt)
  {
    const int rc = by_alloc ? b.alloc(need, sizeof(uint32_t)) : b.grow(need, sizeof(uint32_t), slack);
    if (verdict(what, rc, b.p && b.cap >= need, !b.p && b.cap == 0)) return 1;
    if (rc != WS_OK) continue;
    EXPECT(b.as<uint32_t>() == b.p && const_cast<const DevBuf &>(b).as<uint32_t>() == b.p);
    EXPECT(slack == DevBuf::EIGHTH && !by_alloc ? b.cap == need + need / 8 : b.cap == need); // exact stays exact
    const void *before = b.p;
    EXPECT(b.grow(need, sizeof(uint32_t), slack) == WS_OK && b.p == before); // what fits is left alone
    EXPECT(b.grow(4 * need, sizeof(uint32_t), slack) == WS_OK && b.p && b.cap >= 4 * need);
    b.release(); // (the second attempt starts empty, like the first)
  }
  b.release();
  b.release();
  EXPECT(!b.p && b.cap == 0);
  return 0;
}

static int host_block(const char *what, HostBlock::Kind kind, bool zero)
{
  const size_t need = 100;
  HostBlock b;
  for (int attempt = 0; attempt < 2; ++attempt)
  {
    const int rc = b.grow(need, sizeof(uint64_t), kind, zero);
    if (verdict(what, rc, b.p && b.cap >= need && (kind == HostBlock::MAPPED) == (b.dev != nullptr), !b.p && !b.dev && b.cap == 0)) return 1;
    if (rc != WS_OK) continue;
    EXPECT(b.cap == need);
    uint64_t *w = b.as<uint64_t>();
    if (zero)
      for (size_t i = 0; i < need; ++i) EXPECT(w[i] == 0);
    w[need - 1] = 7; // the block is the host's to write
    EXPECT(b.dev_as<uint64_t>() == b.dev);
    const void *before = b.p;
    EXPECT(b.grow(need, sizeof(uint64_t), kind, zero) == WS_OK && b.p == before);
    EXPECT(b.grow(2 * need, sizeof(uint64_t), kind, zero) == WS_OK && b.p && b.cap >= 2 * need);
    b.release();
  }
  b.release();
  b.release();
  EXPECT(!b.p && !b.dev && b.cap == 0);
  return 0;
}

static int dev_counter(const char *what, bool on_device)
{
  DevCounter c;
  for (int attempt = 0; attempt < 2; ++attempt)
  {
    const int rc = c.alloc(2, on_device);
    if (verdict(what, rc, c.host && on_device == (c.dev != nullptr), !c.host && !c.dev)) return 1;
    if (rc != WS_OK) continue;
    const void *dev = c.dev, *host = c.host;
    EXPECT(c.alloc(2, on_device) == WS_OK && c.dev == dev && c.host == host); // allocated once
    c.release();
  }
  c.release();
  c.release();
  EXPECT(!c.host && !c.dev);
  return 0;
}

int main()
{
  if (dev_buf("DevBuf::alloc", true, DevBuf::EXACT) || dev_buf("DevBuf::grow exact", false, DevBuf::EXACT) ||
      dev_buf("DevBuf::grow with slack", false, DevBuf::EIGHTH) || host_block("HostBlock pinned", HostBlock::PINNED, false) ||
      host_block("HostBlock mapped", HostBlock::MAPPED, false) || host_block("HostBlock mapped, zeroed", HostBlock::MAPPED, true) ||
      dev_counter("DevCounter", true) || dev_counter("DevCounter, pinned half only", false))
    return 1;
  printf("ok: %d allocations succeeded, %d failed\n", g_ok, g_failed);
  return 0;
}
