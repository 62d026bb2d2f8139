// source_state.hip — SourceState of source_state.h and the two host forms that the source kernels' launch interface declares
// (kernels.h): host code only, no HIP runtime call, the arithmetic of rvb_math.h.
#include "source_state.h"
#include "rvb_math.h"

#include <cmath>
#include <cstring>

SourcePatternDev rvb_source_pattern_device_form(const rvb_source_pattern & p)
{
    SourcePatternDev d;
    const v3 n = normalize3(mk3(p.direction[0], p.direction[1], p.direction[2]));       // kernel.cpp:511, with the device's operations
    d.direction[0] = n.x; d.direction[1] = n.y; d.direction[2] = n.z; d.direction[3] = 0.0f;
    for (int b = 0; b < 8; ++b) d.shape[b] = p.shape[b];
    return d;
}

bool rvb_source_table_basis(const rvb_source_orientation & o, float basis[12])
{
    const v3 facing = mk3(o.facing[0], o.facing[1], o.facing[2]), up = mk3(o.up[0], o.up[1], o.up[2]);
    const v3 bx = normalize3(cross3(up, facing));                   // kernel.cpp:538-549 (transform3, make_model), with the device's operations
    const v3 by = cross3(facing, bx);
    const float rows[12] = {bx.x, bx.y, bx.z, 0.0f, by.x, by.y, by.z, 0.0f, facing.x, facing.y, facing.z, 0.0f};
    for (int i = 0; i < 12; ++i) basis[i] = rows[i];
    bool finite = true;
    for (int i = 0; i < 12; ++i) finite = finite && std::isfinite(rows[i]);
    return finite && (bx.x != 0.0f || bx.y != 0.0f || bx.z != 0.0f);
}

static int refuse(std::string & error, const std::string & what) { error = what; return RVB_ERR_INVALID; }

int SourceState::set_patterns(const rvb_source_pattern * new_patterns, uint64_t npatterns, std::string & error)
{
    if (!new_patterns) npatterns = 0;
    std::vector<SourcePatternDev> form;
    for (uint64_t p = 0; p < npatterns; ++p) {
        bool finite = true;
        for (int i = 0; i < 3; ++i) finite = finite && std::isfinite(new_patterns[p].direction[i]);
        for (int b = 0; b < 8; ++b) finite = finite && std::isfinite(new_patterns[p].shape[b]);
        if (!finite) return refuse(error, "rvb_set_source_pattern: pattern " + std::to_string(p) + " holds a value that is not finite");
        form.push_back(rvb_source_pattern_device_form(new_patterns[p]));
        const float * d = form.back().direction;
        // (a zero vector stays zero under normalize3; a length that overflows or underflows in binary32 does not give a unit vector either)
        const float len2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        if (!(len2 > 0.5f && len2 < 2.0f))
            return refuse(error, "rvb_set_source_pattern: pattern " + std::to_string(p) + " has a direction of zero length (or one binary32 cannot normalise)");
    }
    only(PATTERNS);
    if (form.size() == patterns.size() && (form.empty() || !std::memcmp(form.data(), patterns.data(), form.size() * sizeof(SourcePatternDev))))
        return RVB_OK;
    patterns.swap(form);
    patterns_dirty = true;
    return RVB_OK;
}

int SourceState::set_table(const float * new_table, const rvb_source_orientation * orientations, uint64_t norientations, std::string & error)
{
    if (!new_table) {
        only(PATTERNS);
        return RVB_OK;
    }
    if (!orientations || norientations == 0) return refuse(error, "rvb_set_source_table: a table without orientations");
    const size_t table_floats = (size_t) (RVB_HRTF_ROWS - 1) * 8;
    for (size_t i = 0; i < table_floats; ++i)
        if (!std::isfinite(new_table[i]))
            return refuse(error, "rvb_set_source_table: row " + std::to_string(i / 8) + " of the table holds a value that is not finite");
    std::vector<float> new_bases(12 * (size_t) norientations);
    for (uint64_t p = 0; p < norientations; ++p) {
        bool finite = true;
        for (int i = 0; i < 3; ++i) finite = finite && std::isfinite(orientations[p].facing[i]) && std::isfinite(orientations[p].up[i]);
        if (!finite) return refuse(error, "rvb_set_source_table: orientation " + std::to_string(p) + " holds a value that is not finite");
        if (!rvb_source_table_basis(orientations[p], new_bases.data() + 12 * p))
            return refuse(error, "rvb_set_source_table: orientation " + std::to_string(p) + ": normalize3(cross3(up, facing)) is zero or not finite");
    }
    only(TABLE);
    table.assign(new_table, new_table + table_floats);
    bases.swap(new_bases);
    table_dirty = true;
    return RVB_OK;
}

int SourceState::check_counts(const char * who, uint64_t npairs, std::string & error) const
{
    if (patterns.size() > 1 && patterns.size() != npairs)
        return refuse(error, std::string(who) + ": " + std::to_string(patterns.size()) + " source patterns for " + std::to_string(npairs) +
                             " pair(s): one for all pairs, or one per pair (rvb_set_source_pattern)");
    if (norientations() > 1 && norientations() != npairs)
        return refuse(error, std::string(who) + ": " + std::to_string(norientations()) + " source orientations for " +
                             std::to_string(npairs) + " pair(s): one for all pairs, or one per pair (rvb_set_source_table)");
    return RVB_OK;
}
