// Stage 1's text, made from a chunk's reads and the device's records: the TSV rows and the FASTA of the trimmed reads.  Host code
// without HIP (stage1_format.cpp builds with a plain C++ compiler); stage1.cpp's formatter threads and the bdg_format_* entry
// points share it.  A *_bound is the size of the block the matching write_* may fill: it must never be too small.
#pragma once

#include "../../include/badger_hip.h"

#include <algorithm>
#include <cstddef>

struct RowStats {
    uint64_t reads = 0, bc = 0, pt = 0, r1 = 0, first_pt = ~0ull, first_r1 = ~0ull, wl = 0;
    RowStats& operator+=(const RowStats& s)
    {
        reads += s.reads; bc += s.bc; pt += s.pt; r1 += s.r1; wl += s.wl;
        first_pt = std::min(first_pt, s.first_pt); first_r1 = std::min(first_r1, s.first_r1);
        return *this;
    }
};

// A chunk's whitelist calls (bdg_format_rows_wl): per read the match's answer, and the whitelist in the caller's order;
// k > 0: also the k slots of the top-k match per read (bdg_format_rows_wlk)
struct WlCalls {
    const uint32_t* idx; const uint8_t* ed; const uint16_t* ties;
    const uint32_t* wl; uint32_t nw;
    uint32_t k = 0; const uint32_t* cidx = nullptr; const uint8_t* ced = nullptr;
};

struct TrimStats {
    uint64_t reads = 0, tso = 0, bases = 0, cut = 0, dropped = 0, cut_bases = 0, no_cell = 0, not_kept = 0, no_anchor = 0;
    TrimStats& operator+=(const TrimStats& s)
    {
        reads += s.reads; tso += s.tso; bases += s.bases; cut += s.cut; dropped += s.dropped; cut_bases += s.cut_bases;
        no_cell += s.no_cell; not_kept += s.not_kept; no_anchor += s.no_anchor;
        return *this;
    }
};

// stage 2's answers for the reads of a chunk (bdg_format_trimmed_tags): the cell, the molecule's code and its read count (mol may
// be null), a filter (may be null)
struct Tags {
    const uint32_t* rank; const uint8_t* has; const uint32_t* mol; const uint32_t* mol_reads; const uint8_t* keep;
    Tags at(uint64_t g0) const { return Tags{ rank + g0, has + g0, mol ? mol + g0 : nullptr, mol_reads ? mol_reads + g0 : nullptr, keep ? keep + g0 : nullptr }; }
};

// upper bound of the text of a chunk's rows (+ the headers that fall inside it)
uint64_t rows_bound(const bdg_ingest_chunk* ch, const bdg_extract_rec* recs, uint32_t header_every, size_t header_len,
                    const WlCalls* wc = nullptr);
// rows of a chunk whose first read is read g0 of the input; header_every > 0: the header line goes in front of every read
// whose index is a multiple of it
char* write_rows(const bdg_ingest_chunk* ch, const bdg_extract_rec* recs, char* o, uint64_t g0, uint32_t header_every,
                 const char* header, size_t header_len, RowStats& st, const WlCalls* wc = nullptr);
// upper bound of the FASTA text of a chunk's trimmed reads
uint64_t trimmed_bound(const bdg_ingest_chunk* ch, const bdg_extract_rec* recs, const bdg_trim_rec* tr, bool with_wl, bool with_ch = false,
                       bool with_tags = false);
// ">id\tCR:Z:barcode\tUR:Z:UMI\tST:A:strand[\tCB:Z:whitelist barcode]\n" cDNA in mRNA sense "\n" per read with BDG_TRIM_EMIT
// with cm (the chunk's chimera records): a read with a hit ends at its cut and says so in a last field "\tCH:Z:kind,edits";
// one whose cut is its cDNA's first column is left out
// with tg (stage 2's answers): a read without a cell, or one the filter drops, is left out; the others get "\tCB:Z:cell" and, with
// a molecule, "\tUB:Z:molecule\tRN:i:reads" in front of the CH field
char* write_trimmed(const bdg_ingest_chunk* ch, const bdg_extract_rec* recs, const bdg_trim_rec* tr, const bdg_chimera_rec* cm,
                    const WlCalls* wc, char* o, TrimStats& st, const Tags* tg = nullptr);
