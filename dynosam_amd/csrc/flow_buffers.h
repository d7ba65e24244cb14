// The buffers of the frontend library (dynoflow.hip): grow-only device buffers, the pinned host buffer, a context's events, and the packed
// round trip.  This header includes nothing: size_t, uint8_t and the HIP runtime's types, constants and hipMalloc, hipFree, hipHostMalloc,
// hipHostFree, hipMemcpyAsync, hipEventCreate, hipEventDestroy are its includer's - dynoflow.hip has the runtime's, flow_buffers_check.cpp
// has stand-ins over malloc and memcpy that can be told to fail (no GPU).
#pragma once

struct NoCopy { NoCopy() = default; NoCopy(const NoCopy&) = delete; NoCopy& operator=(const NoCopy&) = delete; };

// Device buffer of n elements.  After a failed allocation it is {nullptr, 0}: a buffer that is not there is never "large enough".
template <class T>
struct DB : NoCopy {
  T* p = nullptr;
  size_t n = 0;
  ~DB() { if (p) (void)hipFree(p); }
  bool alloc(size_t c) {   // exactly c elements, whatever was there before (contents are not kept)
    if (p) (void)hipFree(p);
    p = nullptr; n = 0;
    if (hipMalloc((void**)&p, sizeof(T) * (c ? c : 1)) != hipSuccess) { p = nullptr; return false; }
    n = c; return true;
  }
  // grow-only, to exactly c: buffers sized by the image or by a tensor shape, which change rarely and then by a lot
  bool need(size_t c) { return (p && n >= c) || alloc(c); }
  // grow-only, to c + c / 2: per-call counts of points, problems and hypotheses, which creep upwards from call to call
  bool need_room(size_t c) { return (p && n >= c) || alloc(c + c / 2); }
};

// grow-only pinned host buffer
struct PinBuf {
  uint8_t* p = nullptr;
  size_t cap = 0;
  ~PinBuf() { if (p) (void)hipHostFree(p); }
  bool need(size_t bytes) {
    if (bytes <= cap) return true;
    if (p) (void)hipHostFree(p);
    p = nullptr; cap = 0;
    const size_t c = bytes + bytes / 2 + 4096;
    if (hipHostMalloc((void**)&p, c, hipHostMallocDefault) != hipSuccess) { p = nullptr; return false; }
    cap = c;
    return true;
  }
};

// N events: ready() creates the missing ones, the destructor destroys what exists
template <int N>
struct Events : NoCopy {
  hipEvent_t e[N] = {};
  ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
  bool ready() { for (hipEvent_t& x : e) if (!x && hipEventCreate(&x) != hipSuccess) { x = nullptr; return false; } return true; }
  hipEvent_t operator[](int k) const { return e[k]; }
};

// One device buffer mirrored by one pinned host buffer.  A call lays its fields out with put(), fills the host side, sends [0, bytes) up,
// runs its kernels on the device side and brings [from, to) back to the same offsets of the host side.
struct Packed {
  DB<uint8_t> dev;
  PinBuf pin;
  size_t end = 0;   // the layout cursor: where the next field goes
  Packed& rewind() { end = 0; return *this; }
  // offset of a field at a multiple of `align` (a power of two); the cursor moves past the field padded to `align`
  size_t put(size_t bytes, size_t align = 16) { const size_t o = (end + align - 1) & ~(align - 1); end = o + ((bytes + align - 1) & ~(align - 1)); return o; }
  bool need(size_t device_bytes, size_t host_bytes) { return dev.need_room(device_bytes) && pin.need(host_bytes); }
  bool up(size_t bytes, hipStream_t st) { return hipMemcpyAsync(dev.p, pin.p, bytes, hipMemcpyHostToDevice, st) == hipSuccess; }
  bool down(size_t from, size_t to, hipStream_t st) { return hipMemcpyAsync(pin.p + from, dev.p + from, to - from, hipMemcpyDeviceToHost, st) == hipSuccess; }
  template <class T = uint8_t> T* d(size_t o) const { return reinterpret_cast<T*>(dev.p + o); }
  template <class T = uint8_t> T* h(size_t o) const { return reinterpret_cast<T*>(pin.p + o); }
};
