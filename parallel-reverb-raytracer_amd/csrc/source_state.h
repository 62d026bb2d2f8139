// source_state.h — the host half of a context's source directivity (rvb_set_source_pattern / rvb_set_source_table of
// include/rvb_capi.h): what the two setters accept and refuse, which of the two is on, and what the next trace or re-shade has to
// upload.  Defined in source_state.hip, which makes no HIP runtime call and holds no kernel: a host program can link it
// (tests/cpp/source_state.cpp does).  The device half, SourceDirectivity of ctx.h, is built on it; the entry points and the launches
// are in source.hip.
#pragma once

#include "kernels.h"

#include <string>
#include <vector>

#pragma GCC visibility push(hidden)

// What shades the records at the source end — a source has one directivity at a time —: nothing, the patterns of rvb_set_source_pattern
// in their device form, or the table of rvb_set_source_table with this many orientations.
struct SourceShading {
    std::vector<SourcePatternDev> patterns;
    uint32_t table_orientations = 0;
    bool off() const { return patterns.empty() && table_orientations == 0; }
};

// The setters take the arguments of the C entry points, return an RVB_* code and leave the text of a refusal in `error`; a refused
// call leaves the state exactly as it was.  Everything here is what the NEXT trace or re-shade applies: what is on the device stays
// until that one uploads (a kept trace may reflect it, and rvb_relisten shades with it).
struct SourceState {
    std::vector<SourcePatternDev> patterns;     // rvb_set_source_pattern, in device form; empty: off
    std::vector<float> table;                   // rvb_set_source_table: [360 * 180][8]; empty: off
    std::vector<float> bases;                   // ... and the bases of its orientations (rvb_source_table_basis): [norientations][12]
    // not on the device yet.  The same patterns set again — a pipeline sets them per job — are not uploaded again; a table always is.
    bool patterns_dirty = false, table_dirty = false;

    uint32_t norientations() const { return table.empty() ? 0u : (uint32_t) (bases.size() / 12); }
    bool patterns_need_upload() const { return patterns_dirty && !patterns.empty(); }
    bool table_needs_upload() const { return table_dirty && !table.empty(); }
    // what the traces and re-shades that follow apply
    SourceShading shading() const
    {
        SourceShading s;
        s.patterns = patterns;
        s.table_orientations = norientations();
        return s;
    }

    // new_patterns == NULL (or npatterns == 0): no patterns.  An accepted call turns the table off.  direction[3] is not inspected.
    int set_patterns(const rvb_source_pattern * new_patterns, uint64_t npatterns, std::string & error);
    // An accepted call turns the patterns off; new_table == NULL: the table off, the patterns as they are.  Only the first
    // (RVB_HRTF_ROWS - 1) * 8 floats of a table are read.
    int set_table(const float * new_table, const rvb_source_orientation * orientations, uint64_t norientations, std::string & error);
    // "n orientations / patterns for npairs pairs": one for all pairs, or one per pair
    int check_counts(const char * who, uint64_t npairs, std::string & error) const;

private:
    enum Which { PATTERNS, TABLE };
    // One directivity at a time: every accepted call of either setter passes here, and whatever is not `on` is off from then on.
    void only(Which on)
    {
        if (on != PATTERNS) patterns.clear();
        if (on != TABLE) { table.clear(); bases.clear(); }
    }
};

#pragma GCC visibility pop
