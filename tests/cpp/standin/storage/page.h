// storage/page.h — TEST INFRASTRUCTURE: stand-in for the store's header of
// this name, used by tests/cpp/gen_integration.py only where the reference
// tree is absent, so that INTEGRATION.md's snippets still build and run.
//
// It states the part of that header's surface the call-site snippets and
// include/eloqstore/page_checksum.h meet: the width of the page header that
// holds the checksum, the pool's chunk alignment, and the two single-page functions whose bodies stay
// with the store (the harness defines them).  Where the
// reference tree is present the snippets compile against its own header
// instead (tests/test_integration_compile.py).
#pragma once

#include <unistd.h>

#include <cstddef>
#include <cstdint>
#include <string_view>

namespace eloqstore {

constexpr uint8_t checksum_bytes = 8;

// alignment of the page pool's chunks: the system's memory page size
inline const size_t page_align = static_cast<size_t>(sysconf(_SC_PAGESIZE));

void SetChecksum(std::string_view blob);
bool ValidateChecksum(std::string_view blob);

}  // namespace eloqstore
