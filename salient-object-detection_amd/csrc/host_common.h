// What the host halves of the codecs share (csrc/jpeg_host.h, csrc/png_host.h): plain C++, no HIP, so that the stand-alone
// sanitizer programs under scripts/ compile it as well.
#pragma once
#include <stddef.h>

namespace sm {

inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

}  // namespace sm
