// What the stand-alone host twins (post_math_main.cpp, seed_math_main.cpp) share beside their arithmetic: `PROGRAM IN OUT [libm|device]`,
// arrays read from and written to flat little-endian files, and the paths out of a failure (a message on stderr, exit status 2).
// Include it behind device_trig_twin.hpp: the third argument sets g_device_trig.
#pragma once
#include <cstdio>
#include <cstring>
#include <vector>

template <class T> static bool get(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}
template <class T> static bool put(FILE* f, const std::vector<T>& v) { return v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

// the arguments checked, the trig mode set, IN opened -> NULL: return 2
static FILE* twin_open(int argc, char** argv) {
  if (argc != 3 && argc != 4) { std::fprintf(stderr, "usage: %s IN OUT [libm|device]\n", argv[0]); return nullptr; }
  if (argc == 4) {
    if (std::strcmp(argv[3], "device") != 0 && std::strcmp(argv[3], "libm") != 0) { std::fprintf(stderr, "unknown trig mode %s\n", argv[3]); return nullptr; }
    g_device_trig = std::strcmp(argv[3], "device") == 0;
  }
  FILE* in = std::fopen(argv[1], "rb");
  if (!in) std::fprintf(stderr, "cannot open %s\n", argv[1]);
  return in;
}
// IN closed; ok: every get succeeded -> false: return 2
static bool twin_read(FILE* in, bool ok, char** argv) {
  std::fclose(in);
  if (!ok) std::fprintf(stderr, "%s is truncated\n", argv[1]);
  return ok;
}
// OUT opened -> NULL: return 2
static FILE* twin_create(char** argv) {
  FILE* out = std::fopen(argv[2], "wb");
  if (!out) std::fprintf(stderr, "cannot write %s\n", argv[2]);
  return out;
}
// OUT closed; ok: every put succeeded -> the exit status, "<name>: ok" on stdout with 0
static int twin_done(FILE* out, bool ok, char** argv, const char* name) {
  if (std::fclose(out) != 0 || !ok) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
  std::printf("%s: ok\n", name);
  return 0;
}
