// bvh_dump — runs rvb_build_scene (csrc/bvh_build.hip, host code) on a scene read from two binary files and writes what it built:
//   bvh_dump <triangles.bin> <vertices.bin> <nsurfaces> <out directory>
// triangles.bin: rvb_triangle records (32 B), vertices.bin: rvb_float3 records (16 B).  Written: nodes.bin (BvhNode), tris.bin (BvhTri, leaf
// order), shade.bin (TriShade, by original index), leafpos.bin (uint32), meta.txt ("depth stack_need pad" with pad as a bit pattern) and
// error.txt (the builder's error text, empty on success).  Exit status 0 whenever the builder returned, 2 on a usage or file error.
// tests/test_bvh_host.py builds and drives it; no GPU, nothing loaded into Python.
#include "bvh.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

template <class T>
bool read_records(const char * path, std::vector<T> & out)
{
    FILE * f = std::fopen(path, "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    bool ok = bytes >= 0 && bytes % (long) sizeof(T) == 0;
    if (ok) {
        out.resize((size_t) bytes / sizeof(T));
        ok = out.empty() || std::fread(out.data(), sizeof(T), out.size(), f) == out.size();
    }
    std::fclose(f);
    return ok;
}

bool write_bytes(const std::string & path, const void * p, size_t bytes)
{
    FILE * f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = bytes == 0 || std::fwrite(p, 1, bytes, f) == bytes;
    return std::fclose(f) == 0 && ok;
}

}  // namespace

int main(int argc, char ** argv)
{
    if (argc != 5) {
        std::fprintf(stderr, "usage: bvh_dump <triangles.bin> <vertices.bin> <nsurfaces> <out directory>\n");
        return 2;
    }
    std::vector<rvb_triangle> triangles;
    std::vector<rvb_float3> vertices;
    if (!read_records(argv[1], triangles) || !read_records(argv[2], vertices)) {
        std::fprintf(stderr, "bvh_dump: cannot read the scene files\n");
        return 2;
    }
    const unsigned long long nsurfaces = std::strtoull(argv[3], nullptr, 10);
    const std::string dir = std::string(argv[4]) + "/";
    BuiltScene built;
    const std::string error = rvb_build_scene(triangles.data(), triangles.size(), vertices.data(), vertices.size(), nsurfaces, built);
    uint32_t pad_bits;
    std::memcpy(&pad_bits, &built.pad, sizeof(pad_bits));
    const std::string meta = std::to_string(built.depth) + " " + std::to_string(built.stack_need) + " " + std::to_string(pad_bits) + "\n";
    bool ok = write_bytes(dir + "error.txt", error.data(), error.size());
    ok = write_bytes(dir + "meta.txt", meta.data(), meta.size()) && ok;
    ok = write_bytes(dir + "nodes.bin", built.nodes.data(), built.nodes.size() * sizeof(BvhNode)) && ok;
    ok = write_bytes(dir + "tris.bin", built.tris.data(), built.tris.size() * sizeof(BvhTri)) && ok;
    ok = write_bytes(dir + "shade.bin", built.shade.data(), built.shade.size() * sizeof(TriShade)) && ok;
    ok = write_bytes(dir + "leafpos.bin", built.leafpos.data(), built.leafpos.size() * sizeof(uint32_t)) && ok;
    if (!ok) {
        std::fprintf(stderr, "bvh_dump: cannot write to %s\n", argv[4]);
        return 2;
    }
    return 0;
}
