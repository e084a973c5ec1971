// vlr_callsfile.cpp — calls file in: the calls-BCF reader (open_calls, read_call_records) and the record passes of its three consumers,
// `filter-calls control-fdr`, `filter-calls posterior-odds` and `estimate mutational-burden`.  The container itself (header opener,
// record framer, the walk over a record's shared block, typed values, float sentinels) is vlr_hostio.h's; this file says what a
// calls record's fields mean.
#include <limits>
#include <unordered_set>

#include "vlr_hostio.h"

using namespace vlr_hostio;

// ================================================================================================ filter-calls control-fdr
// The whole of `varlociraptor filter-calls control-fdr` behind the ABI (reference src/filtration/fdr.rs:36-158,
// src/utils/mod.rs:169-374, record typing src/utils/collect_variants.rs:44-304): calls BCF in -> kept records out, the threshold
// search on the device (vlr_fdr_threshold).  The Python restatement the tests compare with: varlociraptor_amd/fdr.py.
extern "C" int vlr_fdr_threshold(int device, const double* ln_prob, int64_t n, int smart, double alpha_ln, double* threshold, int* status);
namespace {
constexpr double kNumericalEpsilon = 1e-3;  // utils/mod.rs:40
int vk_of(const std::string& s) {
    static const char* const n[] = {"SNV", "MNV", "INS", "DEL", "BND", "INV", "DUP", "REP", "REF", "METH"};
    for (int i = 0; i < 10; ++i) if (s == n[i]) return i;
    return -1;
}
bool valid_del(const std::string& r, const std::string& a) { return a == "<DEL>" || (r.size() > a.size() && r.compare(0, a.size(), a) == 0 && a.size() == 1); }
bool valid_ins(const std::string& r, const std::string& a) { return a == "<INS>" || (r.size() < a.size() && a.compare(0, r.size(), r) == 0 && r.size() == 1); }
bool is_type(const VarType& v, const TypeFilter& f) {  // Variant::is_type (variants/model/mod.rs)
    if (v.kind < 0) return false;
    if (f.kind < 0) return true;
    if (v.kind != f.kind) return false;
    return !f.has_range || (f.lo <= v.len && v.len < f.hi);
}
double lse(const std::vector<double>& v) {  // bio LogProb::ln_sum_exp: the maximum apart, ln_1p of the others
    if (v.empty()) return -INFINITY;
    size_t im = 0;
    for (size_t i = 1; i < v.size(); ++i)
        if (v[i] > v[im]) im = i;
    const double m = v[im];
    if (m == -INFINITY) return m;
    double s = 0.0;
    for (size_t i = 0; i < v.size(); ++i)
        if (i != im && v[i] != -INFINITY) s += std::exp(v[i] - m);
    return m + std::log1p(s);
}
double ln_one_minus_exp(double p) { return p < 0.0 ? (p < -0.693 ? std::log1p(-std::exp(p)) : std::log(-std::expm1(p))) : -INFINITY; }
std::string event_tag(const char* event) {  // Event::tag_name("PROB") (lib.rs:52-54)
    std::string t = "PROB_";
    for (const char* q = event; *q; ++q) t.push_back((char)toupper((unsigned char)*q));
    return t;
}
// the INFO tags a consumer wants from read_call_records, in the order it names them first (CallRec::prob is indexed by id)
struct TagSet {
    std::vector<std::string> names;
    int id(const std::string& name) {
        for (size_t i = 0; i < names.size(); ++i) if (names[i] == name) return (int)i;
        names.push_back(name);
        return (int)names.size() - 1;
    }
};
// what the two filters write: the input's header bytes as they are, then the kept records byte for byte (`body`), as BGZF
int write_kept_records(const char* out_path, const CallsFile& cf, const std::vector<uint8_t>& body, int n_threads) {
    const std::vector<uint8_t> header_bytes(cf.data.data(), cf.data.data() + cf.header_bytes);
    std::string err;
    if (!write_bgzf_file(out_path, {&header_bytes, &body}, n_threads, 6, err)) return ifail(VLR_ERR_INVALID_ARGUMENT, "%s", err.c_str());
    return VLR_OK;
}
}  // namespace

namespace vlr_hostio VLR_HIDDEN {

// (type, length) per ALT allele as collect_variants types it (collect_variants.rs:44-304)
bool variant_types(const CallRec& r, std::vector<VarType>& out, std::string& err) {
    out.clear();
    if (!r.svtype.empty()) {
        const std::string& sv = r.svtype;
        if (sv == "INV" || sv == "DUP") {
            VarType v;
            if (r.alts.size() == 1 && r.has_end) { v.kind = sv == "INV" ? VK_INV : VK_DUP; v.len = r.end0 + 1 - r.pos0; }
            out.push_back(v);
        } else if (sv == "BND") {
            for (size_t i = 0; i < r.alts.size(); ++i) out.push_back(VarType{VK_BND, 0});
        } else if (sv == "INS") {
            VarType v;
            if (!r.alts.empty() && r.alts[0] != "<INS>" && valid_ins(r.ref, r.alts[0])) { v.kind = VK_INS; v.len = (int64_t)r.alts[0].size() - (int64_t)r.ref.size(); }
            out.push_back(v);
        } else if (sv == "DEL") {
            int64_t svlen;
            if (r.has_svlen && !r.svlen.empty() && r.svlen[0] >= 0) svlen = r.svlen[0];
            else if (!r.has_svlen && r.has_end) svlen = r.end0 - (r.pos0 + 1);  // collect_variants.rs:196-199
            else { err = "missing SVLEN or END"; return false; }
            VarType v;
            if (!r.alts.empty() && valid_del(r.ref, r.alts[0])) { v.kind = VK_DEL; v.len = svlen; }
            out.push_back(v);
        }
        return true;
    }
    for (size_t i = 0; i < r.alts.size(); ++i) {
        const std::string& a = r.alts[i];
        VarType v;
        if (a == "<*>") v = VarType{VK_REF, 0};
        else if (a == "<DEL>") { if (r.has_svlen && i < r.svlen.size() && r.svlen[i] >= 0) v = VarType{VK_DEL, r.svlen[i]}; }
        else if (a == "<METH>") v = VarType{VK_METH, 0};
        else if (!a.empty() && a[0] == '<') {}
        else if (a.size() == 1 && r.ref.size() == 1) v = VarType{VK_SNV, 1};
        else if (a.size() == r.ref.size()) v = VarType{VK_MNV, (int64_t)a.size()};
        else if (valid_del(r.ref, a)) v = VarType{VK_DEL, (int64_t)r.ref.size() - (int64_t)a.size()};
        else if (valid_ins(r.ref, a)) v = VarType{VK_INS, (int64_t)a.size() - (int64_t)r.ref.size()};
        else v = VarType{VK_REP, 0};
        out.push_back(v);
    }
    return true;
}
// utils/mod.rs:177-212: ln-sum over the given PROB_* tags per (typed) variant; NaN = None
void tags_prob_sum(const CallRec& r, const std::vector<VarType>& types, const std::vector<int>& tags, const TypeFilter& tf, std::vector<double>& out) {
    std::vector<const VarType*> variants;
    for (auto& v : types) if (v.kind >= 0) variants.push_back(&v);
    std::vector<std::vector<double>> acc(variants.size());
    for (int t : tags) {
        const std::vector<double>& vals = r.prob[(size_t)t];
        for (size_t i = 0; i < variants.size() && i < vals.size(); ++i) {
            const double p = vals[i];
            if (p != p || !is_type(*variants[i], tf)) continue;
            acc[i].push_back(-p * std::log(10.0) / 10.0);
        }
    }
    out.clear();
    for (auto& probs : acc) {
        if (probs.empty()) { out.push_back(NAN); continue; }
        double s = lse(probs);
        if (0.0 < s && s <= kNumericalEpsilon) s = 0.0;  // cap_numerical_overshoot
        out.push_back(s);
    }
}

int open_calls(const char* in_path, int n_threads, CallsFile& f) {
    std::string err;
    if (!load_inflated(in_path, f.data, n_threads, err)) return ifail(VLR_ERR_INVALID_ARGUMENT, "%s", err.c_str());
    const BcfHead head = bcf_head(f.data.data(), f.data.size(), f.header_bytes, f.h);
    if (head == BCF_SHORT || head == BCF_NOT) return ifail(VLR_ERR_INVALID_ARGUMENT, "%s is not a BCF file", in_path);
    if (head == BCF_PARTIAL) return ifail(VLR_ERR_INVALID_ARGUMENT, "truncated BCF header in %s", in_path);
    const std::string& text = f.h.text;
    const size_t c = text.find("#CHROM");
    if (c != std::string::npos && (c == 0 || text[c - 1] == '\n')) {
        size_t e = text.find('\n', c);
        if (e == std::string::npos) e = text.size();
        int col = 0;
        for (size_t q = c; q <= e;) {
            size_t t = text.find('\t', q);
            if (t == std::string::npos || t > e) t = e;
            if (col >= 9) f.samples.push_back(text.substr(q, t - q));
            ++col;
            q = t + 1;
        }
    }
    return VLR_OK;
}
// the records of an opened calls file: alleles, the float INFO tags `tag_names` (CallRec::prob in that order), EVENT, SVTYPE, SVLEN,
// END; with_ann_af: INFO/ANN and FORMAT/AF as well
int read_call_records(const char* in_path, CallsFile& f, const std::vector<std::string>& tag_names, bool with_ann_af) {
    const Header& h = f.h;
    std::vector<int> key_tag(h.dict.size(), -1);  // dictionary index -> 0.. wanted tag, -2 EVENT, -3 SVTYPE, -4 SVLEN, -5 END, -6 ANN, -7 AF
    for (size_t k = 0; k < h.dict.size(); ++k) {
        for (size_t t = 0; t < tag_names.size(); ++t) if (h.dict[k] == tag_names[t]) key_tag[k] = (int)t;
        if (h.dict[k] == "EVENT") key_tag[k] = -2;
        else if (h.dict[k] == "SVTYPE") key_tag[k] = -3;
        else if (h.dict[k] == "SVLEN") key_tag[k] = -4;
        else if (h.dict[k] == "END") key_tag[k] = -5;
        else if (with_ann_af && h.dict[k] == "ANN") key_tag[k] = -6;
        else if (with_ann_af && h.dict[k] == "AF") key_tag[k] = -7;
    }
    std::vector<CallRec>& recs = f.recs;
    static const char* const kWalkText[] = {"", "truncated BCF record in %s", "bad ID field in %s", "bad allele in %s", "bad FILTER field in %s", "bad INFO field in %s"};
    const uint8_t* const d = f.data.data();
    const size_t n = f.data.size();
    size_t p = f.header_bytes;
    while (p + 8 <= n) {
        size_t rec_end;
        uint32_t ls;
        if (!bcf_frame(d, n, p, rec_end, &ls) || ls < 24) return ifail(VLR_ERR_INVALID_ARGUMENT, "truncated BCF record in %s", in_path);
        CallRec r;
        r.raw = d + p; r.raw_len = rec_end - p;
        r.prob.resize(tag_names.size());
        BcfSite site;
        const BcfWalk w = bcf_walk_shared(d + p, d + rec_end, site,
            [](const Typed&) {},
            [&](uint32_t a, const Typed& t) {
                std::string s((const char*)t.data, t.n);
                if (a == 0) r.ref = s; else r.alts.push_back(s);
            },
            [&](int32_t ki, const Typed& val) {
                const int kt = (ki >= 0 && (size_t)ki < key_tag.size()) ? key_tag[(size_t)ki] : -1;
                if (kt >= 0 && val.type == 5) {
                    auto& v = r.prob[(size_t)kt];
                    for (uint32_t i = 0; i < val.n; ++i) {
                        uint32_t bits;
                        memcpy(&bits, val.data + 4 * (size_t)i, 4);
                        if (bcf_float_end_of_vector(bits)) break;
                        float x;
                        memcpy(&x, &bits, 4);
                        v.push_back(bcf_float_missing(bits) ? NAN : (double)x);
                    }
                    if (v.empty()) v.push_back(NAN);  // (a present tag is a list: keeps "tag absent" apart)
                } else if (kt == -2 && val.type == 7) {
                    r.event.assign((const char*)val.data, val.n);
                    while (!r.event.empty() && r.event.back() == '\0') r.event.pop_back();
                    r.has_event = true;
                } else if (kt == -3 && val.type == 7) {
                    r.svtype.assign((const char*)val.data, val.n);
                    while (!r.svtype.empty() && r.svtype.back() == '\0') r.svtype.pop_back();
                } else if (kt == -6 && val.type == 7) {
                    r.ann.assign((const char*)val.data, val.n);
                    while (!r.ann.empty() && r.ann.back() == '\0') r.ann.pop_back();
                    r.has_ann = true;
                } else if ((kt == -4 || kt == -5) && val.type >= 1 && val.type <= 3) {
                    static const int32_t miss[4] = {0, -128, -32768, (int32_t)0x80000000}, eov[4] = {0, -127, -32767, (int32_t)0x80000001};
                    std::vector<int64_t> vals;
                    for (uint32_t i = 0; i < val.n; ++i) {
                        const int32_t x = typed_int(val, i);
                        if (x == eov[val.type]) continue;
                        vals.push_back(x == miss[val.type] ? -1 : (kt == -4 ? std::llabs((long long)x) : (int64_t)x));
                    }
                    if (kt == -4) { r.has_svlen = true; r.svlen = vals; }
                    else if (!vals.empty()) { r.has_end = true; r.end0 = vals[0] - 1; }
                }
            });
        if (w != BCF_WALK_OK) return ifail(VLR_ERR_INVALID_ARGUMENT, kWalkText[w], in_path);
        r.contig = site.contig; r.pos0 = site.pos0;
        if (with_ann_af) {  // FORMAT blocks: key, type descriptor, n_sample vectors
            const uint32_t n_fmt = site.n_fmt, n_sample = site.n_sample;
            const uint8_t* fq = site.shared_end;
            const uint8_t* const fe = d + rec_end;
            static const int size[16] = {0, 1, 2, 4, 0, 4, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0};
            for (uint32_t k = 0; k < n_fmt; ++k) {
                Typed key;
                if (!bcf_typed(fq, fe, key) || key.n != 1 || key.type < 1 || key.type > 3 || fq >= fe) return ifail(VLR_ERR_INVALID_ARGUMENT, "bad FORMAT field in %s", in_path);
                const uint8_t b = *fq++;
                const int type = b & 0xf;
                uint32_t n = b >> 4;
                if (n == 15) {
                    Typed l;
                    if (!bcf_typed(fq, fe, l) || l.n != 1 || l.type < 1 || l.type > 3 || typed_int(l, 0) < 0) return ifail(VLR_ERR_INVALID_ARGUMENT, "bad FORMAT field in %s", in_path);
                    n = (uint32_t)typed_int(l, 0);
                }
                const size_t bytes = (size_t)n * size[type] * n_sample;
                if ((size_t)(fe - fq) < bytes) return ifail(VLR_ERR_INVALID_ARGUMENT, "truncated FORMAT field in %s", in_path);
                const int32_t ki = typed_int(key, 0);
                if (ki >= 0 && (size_t)ki < key_tag.size() && key_tag[(size_t)ki] == -7 && type == 5) {
                    r.has_af = true;
                    r.af.assign(n_sample, std::vector<float>());
                    for (uint32_t sidx = 0; sidx < n_sample; ++sidx)
                        for (uint32_t i = 0; i < n; ++i) {
                            uint32_t bits;
                            memcpy(&bits, fq + 4 * ((size_t)sidx * n + i), 4);
                            if (bcf_float_end_of_vector(bits)) break;
                            float x;
                            memcpy(&x, &bits, 4);
                            r.af[sidx].push_back(bcf_float_missing(bits) ? NAN : x);
                        }
                }
                fq += bytes;
            }
        }
        recs.push_back(std::move(r));
        p = rec_end;
    }
    return VLR_OK;
}
}  // namespace vlr_hostio

extern "C" int vlr_calls_filter_fdr(const char* in_path, const char* out_path, int n_events, const char* const* events, double alpha, uint32_t mode,
                                    const char* vartype, int64_t minlen, int64_t maxlen, int device, int n_threads, int64_t* n_kept, int64_t* n_total) {
    if (!in_path || !out_path || n_events <= 0 || !events) return ifail(VLR_ERR_INVALID_ARGUMENT, "null argument");
    if (!(alpha > 0.0)) return ifail(VLR_ERR_INVALID_ARGUMENT, "alpha must be positive");
    const bool local = (mode & VLR_FDR_MODE_LOCAL) != 0, smart = (mode & VLR_FDR_MODE_SMART) != 0, retain = (mode & VLR_FDR_MODE_RETAIN_ARTIFACTS) != 0;
    n_threads = pick_threads(n_threads);
    TypeFilter tf;
    if (vartype && *vartype) {
        tf.kind = vk_of(vartype);
        if (tf.kind < 0) return ifail(VLR_ERR_INVALID_ARGUMENT, "unknown variant type %s", vartype);
        if (minlen >= 0 || maxlen >= 0) { tf.has_range = true; tf.lo = minlen >= 0 ? minlen : 0; tf.hi = maxlen >= 0 ? maxlen : ((int64_t)1 << 62); }
    }
    std::string err;
    CallsFile cf;
    if (int rc = open_calls(in_path, n_threads, cf)) return rc;
    const Header& h = cf.h;
    // wanted INFO tags: the events' PROB_* (those the header declares, fdr.rs:46-60), PROB_ABSENT, PROB_ARTIFACT
    TagSet tags;
    auto declared = [&](const std::string& name) { return std::find(h.dict.begin(), h.dict.end(), name) != h.dict.end() && h.text.find("##INFO=<ID=" + name + ",") != std::string::npos; };
    std::vector<int> ev_tags;
    for (int i = 0; i < n_events; ++i) {
        const std::string t = event_tag(events[i]);
        if (declared(t)) ev_tags.push_back(tags.id(t));
    }
    if (ev_tags.empty()) return ifail(VLR_ERR_INVALID_ARGUMENT, "invalid FDR control events");  // errors::Error::InvalidFDRControlEvents
    const int t_absent = tags.id("PROB_ABSENT"), t_artifact = tags.id("PROB_ARTIFACT");
    if (int rc = read_call_records(in_path, cf, tags.names, false)) return rc;
    const std::vector<CallRec>& recs = cf.recs;
    const int64_t N = (int64_t)recs.size();
    std::vector<std::vector<VarType>> types((size_t)N);
    for (int64_t i = 0; i < N; ++i)
        if (!variant_types(recs[(size_t)i], types[(size_t)i], err)) return ifail(VLR_ERR_INVALID_ARGUMENT, "%s (record %lld of %s)", err.c_str(), (long long)i, in_path);
    // threshold (fdr.rs:62-141)
    const double alpha_ln = std::log(alpha);
    bool have_thr = false;
    double thr = 0.0;
    if (local) { have_thr = true; thr = alpha < 1.0 ? std::log1p(-alpha) : -INFINITY; }
    else if (alpha != 1.0) {
        std::vector<int> dist_tags;
        if (smart) { dist_tags.push_back(t_absent); if (!retain) dist_tags.push_back(t_artifact); }
        else dist_tags = ev_tags;
        std::vector<double> dist, sums;
        std::unordered_set<std::string> seen;
        for (int64_t i = 0; i < N; ++i) {  // utils/mod.rs:236-270: one entry per breakend event
            const CallRec& r = recs[(size_t)i];
            if (r.has_event) { if (seen.count(r.event)) continue; seen.insert(r.event); }
            tags_prob_sum(r, types[(size_t)i], dist_tags, tf, sums);
            for (double s : sums) if (s == s) dist.push_back(s);
        }
        int status = 0;
        const int rc = vlr_fdr_threshold(device, dist.data(), (int64_t)dist.size(), smart ? 1 : 0, alpha_ln, &thr, &status);
        if (rc != 0) return rc;
        if (status == VLR_FDR_VALUE) have_thr = true;
        else if (status == VLR_FDR_LN_ONE) { have_thr = true; thr = 0.0; }
    }
    // filter_by_threshold (utils/mod.rs:288-374)
    std::vector<int> ftags = ev_tags, absent_tags{t_absent};
    if (smart && retain) ftags.push_back(t_artifact); else absent_tags.push_back(t_artifact);
    std::unordered_map<std::string, bool> decisions;
    std::vector<uint8_t> body;
    int64_t kept = 0;
    std::vector<double> pe, pa;
    for (int64_t i = 0; i < N; ++i) {
        const CallRec& r = recs[(size_t)i];
        tags_prob_sum(r, types[(size_t)i], ftags, tf, pe);
        if (smart) tags_prob_sum(r, types[(size_t)i], absent_tags, tf, pa);
        bool keep_any = false;
        for (size_t v = 0; v < pe.size(); ++v) {
            bool keep;
            auto it = r.has_event ? decisions.find(r.event) : decisions.end();
            if (r.has_event && it != decisions.end()) keep = it->second;
            else {
                const double prob_events = pe[v];
                double p = prob_events;
                if (smart) { const double a = v < pa.size() ? pa[v] : NAN; p = (a == a) ? ln_one_minus_exp(a) : NAN; }
                if (p == p && have_thr) keep = p > thr || relative_eq(p, thr);
                else if (p == p) keep = true;
                else keep = false;
                if (smart) keep = keep && (prob_events == prob_events && prob_events > std::log(0.5));
                if (r.has_event) decisions[r.event] = keep;
            }
            keep_any = keep_any || keep;
        }
        if (keep_any) {
            // The reference removes the alleles that did not pass (filter_calls, utils/mod.rs:382-417: record.remove_alleles) and
            // asserts one filter decision per ALT.  This entry writes kept records byte for byte, which is the same thing for the
            // single-ALT records `call variants` emits; anything else is refused rather than emitted untrimmed.
            if (r.alts.size() > 1 || pe.size() != r.alts.size())
                return ifail(VLR_ERR_UNSUPPORTED, "record %lld of %s has %zu ALT alleles (%zu typed variants): multi-allelic calls files are not supported by control-fdr here",
                             (long long)i, in_path, r.alts.size(), pe.size());
            body.insert(body.end(), r.raw, r.raw + r.raw_len); ++kept;
        }
    }
    if (int rc = write_kept_records(out_path, cf, body, n_threads)) return rc;
    if (n_kept) *n_kept = kept;
    if (n_total) *n_total = N;
    return VLR_OK;
}

// ================================================================================================ filter-calls posterior-odds
// The whole of `varlociraptor filter-calls posterior-odds` behind the ABI (reference src/filtration/posterior_odds.rs:19-82,
// utils/mod.rs:177-226, 382-446): calls BCF in -> kept records out; both ln-sums per typed variant are formed here, the
// Kass-Raftery decisions are made on the device (vlr_posterior_odds_keep, csrc/vlr_callstats.hip).  Deviation: the reference trims
// the removed alleles of a kept record (filter_calls: record.remove_alleles); like control-fdr above this writes kept records byte
// for byte, untrimmed — the same thing for the single-ALT records `call variants` emits.  The Python restatement the tests compare
// with: varlociraptor_amd/odds.py.
namespace {
// (ID, Description) of every PROB_* INFO line in header order (utils::get_event_tags, utils/mod.rs:429-446)
std::vector<std::pair<std::string, std::string>> event_tags_of(const std::string& text) {
    std::vector<std::pair<std::string, std::string>> out;
    size_t p = 0;
    while (p < text.size()) {
        size_t e = text.find('\n', p);
        if (e == std::string::npos) e = text.size();
        const std::string line = text.substr(p, e - p);
        p = e + 1;
        if (line.compare(0, 8, "##INFO=<") != 0) continue;
        const std::string id = attr(line.substr(7), "ID");
        if (id.compare(0, 5, "PROB_") != 0) continue;
        std::string desc;
        const size_t d = line.find("Description=");
        if (d != std::string::npos) {
            size_t b = d + 12, q = line.rfind('>');
            if (q == std::string::npos || q < b) q = line.size();
            desc = line.substr(b, q - b);
            if (!desc.empty() && desc[0] == '"') {  // quoted: up to the closing quote
                const size_t c = desc.find('"', 1);
                desc = desc.substr(1, c == std::string::npos ? std::string::npos : c - 1);
            } else {
                const size_t c = desc.find(',');
                if (c != std::string::npos) desc.resize(c);
            }
        }
        out.emplace_back(id, desc);
    }
    return out;
}
bool ends_with(const std::string& s, const char* suffix) {
    const size_t n = strlen(suffix);
    return s.size() >= n && s.compare(s.size() - n, n, suffix) == 0;
}
}  // namespace

extern "C" int vlr_calls_filter_odds(const char* in_path, const char* out_path, int n_events, const char* const* events, int min_level, int device, int n_threads,
                                     int64_t* n_kept, int64_t* n_total) {
    if (!in_path || !out_path || n_events <= 0 || !events) return ifail(VLR_ERR_INVALID_ARGUMENT, "null argument");
    if (min_level < VLR_ODDS_NONE || min_level > VLR_ODDS_VERY_STRONG) return ifail(VLR_ERR_INVALID_ARGUMENT, "min_level %d outside [0, 4]", min_level);
    n_threads = pick_threads(n_threads);
    CallsFile cf;
    if (int rc = open_calls(in_path, n_threads, cf)) return rc;
    const auto etags = event_tags_of(cf.h.text);
    for (auto& t : etags)  // is_phred_scaled (a missing closing parenthesis passes, for backward compatibility)
        if (!(ends_with(t.second, "(PHRED)") || !ends_with(t.second, ")")))
            return ifail(VLR_ERR_INVALID_ARGUMENT, "Event probabilities are not PHRED scaled, aborting (%s: %s)", t.first.c_str(), t.second.c_str());
    TagSet tags;
    std::vector<int> target_tags, other_tags;
    for (int i = 0; i < n_events; ++i) target_tags.push_back(tags.id(event_tag(events[i])));
    for (auto& t : etags) {
        bool is_event = false;
        for (int i = 0; i < n_events; ++i) is_event = is_event || t.first.compare(5, std::string::npos, events[i]) == 0;  // the name as given
        if (!is_event) other_tags.push_back(tags.id(t.first));
    }
    if (int rc = read_call_records(in_path, cf, tags.names, false)) return rc;
    const std::vector<CallRec>& recs = cf.recs;
    const int64_t N = (int64_t)recs.size();
    const TypeFilter all;
    std::string err;
    std::vector<VarType> types;
    std::vector<double> lt, lo, st, so;
    std::vector<uint8_t> valid;
    std::vector<int64_t> first((size_t)N + 1, 0);
    for (int64_t i = 0; i < N; ++i) {
        if (!variant_types(recs[(size_t)i], types, err)) return ifail(VLR_ERR_INVALID_ARGUMENT, "%s (record %lld of %s)", err.c_str(), (long long)i, in_path);
        tags_prob_sum(recs[(size_t)i], types, target_tags, all, st);
        tags_prob_sum(recs[(size_t)i], types, other_tags, all, so);
        for (size_t v = 0; v < st.size(); ++v) {
            const bool vt = st[v] == st[v], vo = so[v] == so[v];
            lt.push_back(vt ? st[v] : 0.0);
            lo.push_back(vo ? so[v] : 0.0);
            valid.push_back((uint8_t)((vt ? 1 : 0) | (vo ? 2 : 0)));
        }
        first[(size_t)i + 1] = (int64_t)lt.size();
    }
    std::vector<uint8_t> keep(lt.size(), 0);
    if (int rc = vlr_posterior_odds_keep(device, (int64_t)lt.size(), lt.data(), lo.data(), valid.data(), min_level, keep.data())) return rc;
    std::vector<uint8_t> body;
    int64_t kept = 0;
    for (int64_t i = 0; i < N; ++i) {
        bool any = false;
        for (int64_t v = first[(size_t)i]; v < first[(size_t)i + 1]; ++v) any = any || keep[(size_t)v];
        if (any) { body.insert(body.end(), recs[(size_t)i].raw, recs[(size_t)i].raw + recs[(size_t)i].raw_len); ++kept; }
    }
    if (int rc = write_kept_records(out_path, cf, body, n_threads)) return rc;
    if (n_kept) *n_kept = kept;
    if (n_total) *n_total = N;
    return VLR_OK;
}

// ================================================================================================ estimate mutational-burden
// The record pass of `varlociraptor estimate mutational-burden` (reference src/estimation/mutational_burden.rs:18-43, 93-184,
// 482-515) and its reduction on the device (vlr_range_group_lse, csrc/vlr_callstats.hip).  Scaling and output:
// varlociraptor_amd/burden.py, which also holds the numpy restatement the tests compare with.
namespace {
constexpr int kNSignatures = 14;      // DEL METH INS INV DUP BND MNV Complex C>A C>G C>T T>A T>C T>G
constexpr int64_t kUploadPiece = 1 << 16;  // entries per host-to-device copy
bool is_coding(const std::string& ann) {  // is_valid_variant over the ','-separated ANN entries
    size_t p = 0;
    while (p <= ann.size()) {
        size_t e = ann.find(',', p);
        if (e == std::string::npos) e = ann.size();
        bool coding = false;
        int i = 0;
        for (size_t q = p; q <= e; ++i) {
            size_t b = ann.find('|', q);
            if (b == std::string::npos || b > e) b = e;
            if (i == 7) coding = ann.compare(q, b - q, "protein_coding") == 0;
            if (i == 13) coding = coding && b > q;
            q = b + 1;
        }
        if (coding) return true;
        p = e + 1;
    }
    return false;
}
int signature_of(const std::string& ref, const std::string& alt) {  // signatures(); -1: an SNV that is no ACGT substitution
    if (alt == "<DEL>") return 0;
    if (alt == "<INV>") return 3;
    if (alt == "<DUP>") return 4;
    if (alt == "<BND>") return 5;
    if (alt == "<METH>") return 1;
    if (ref.size() == 1 && alt.size() == 1) {
        static const char* const cls[6][2] = {{"CA", "GT"}, {"CG", "GC"}, {"CT", "GA"}, {"TA", "AT"}, {"TC", "AG"}, {"TG", "AC"}};
        for (int c = 0; c < 6; ++c)
            for (int k = 0; k < 2; ++k)
                if (ref[0] == cls[c][k][0] && alt[0] == cls[c][k][1]) return 8 + c;
        return -1;
    }
    if (ref.size() > 1 && alt.size() == 1) return 0;
    if (ref.size() == 1 && alt.size() > 1) return 2;
    if (ref.size() == alt.size() && ref.size() > 1) return 6;
    return 7;
}
double ln_add_exp(double a, double b) {  // bio LogProb::ln_add_exp; NaN in, NaN out
    if (a != a || b != b) return NAN;
    if (b > a) std::swap(a, b);
    if (a == -INFINITY) return a;
    return a + std::log1p(std::exp(b - a));
}
}  // namespace

extern "C" int vlr_calls_mutational_burden(const char* in_path, int n_events, const char* const* events, int n_samples, const char* const* samples, int by_sample,
                                           int n_ranges, const double* lo, const double* hi, int device, int n_threads, double* out_cells, int64_t* n_entries) {
    if (!in_path || n_events <= 0 || !events || n_samples <= 0 || !samples || !lo || !hi || !out_cells) return ifail(VLR_ERR_INVALID_ARGUMENT, "null argument");
    if (n_samples > VLR_MAX_SAMPLES) return ifail(VLR_ERR_INVALID_ARGUMENT, "%d samples: at most %d", n_samples, VLR_MAX_SAMPLES);
    n_threads = pick_threads(n_threads);
    CallsFile cf;
    if (int rc = open_calls(in_path, n_threads, cf)) return rc;
    std::vector<int> sample_col;
    for (int s = 0; s < n_samples; ++s) {
        const auto it = std::find(cf.samples.begin(), cf.samples.end(), std::string(samples[s]));
        if (it == cf.samples.end()) return ifail(VLR_ERR_INVALID_ARGUMENT, "Sample %s not found", samples[s]);
        sample_col.push_back((int)(it - cf.samples.begin()));
    }
    std::vector<int> by_name((size_t)n_samples);  // the reference pushes a record's entries in sample-name order (a BTreeMap's keys, :103-111, :160)
    for (int s = 0; s < n_samples; ++s) by_name[(size_t)s] = s;
    std::stable_sort(by_name.begin(), by_name.end(), [&](int a, int b) { return strcmp(samples[a], samples[b]) < 0; });
    std::vector<std::string> tag_names;
    for (int i = 0; i < n_events; ++i) tag_names.push_back(event_tag(events[i]));
    if (int rc = read_call_records(in_path, cf, tag_names, true)) return rc;
    std::vector<double> vaf, lnp, probs;
    std::vector<int32_t> grp;
    std::vector<int> sig;
    for (size_t i = 0; i < cf.recs.size(); ++i) {
        const CallRec& r = cf.recs[i];
        const std::string contig = (r.contig >= 0 && (size_t)r.contig < cf.h.contigs.size()) ? cf.h.contigs[(size_t)r.contig] : std::string("?");
        if (!r.has_af) return ifail(VLR_ERR_INVALID_ARGUMENT, "record %s:%lld of %s has no FORMAT/AF", contig.c_str(), (long long)r.pos0 + 1, in_path);
        if (!r.has_ann || !is_coding(r.ann)) continue;
        const size_t n_alt = r.alts.size();
        probs.assign(n_alt, -INFINITY);
        bool skip = false;
        for (size_t t = 0; t < tag_names.size() && !skip; ++t) {
            const std::vector<double>& v = r.prob[t];
            if (v.empty()) { skip = true; break; }
            if (v.size() < n_alt) return ifail(VLR_ERR_INVALID_ARGUMENT, "record %s:%lld of %s: %s has %zu values for %zu ALT alleles", contig.c_str(), (long long)r.pos0 + 1,
                                               in_path, tag_names[t].c_str(), v.size(), n_alt);
            for (size_t a = 0; a < n_alt; ++a) probs[a] = ln_add_exp(probs[a], v[a] != v[a] ? NAN : -v[a] * std::log(10.0) / 10.0);
        }
        if (skip) continue;
        sig.resize(n_alt);
        for (size_t a = 0; a < n_alt; ++a) {
            sig[a] = signature_of(r.ref, r.alts[a]);
            if (sig[a] < 0) return ifail(VLR_ERR_INVALID_ARGUMENT, "record %s:%lld of %s: %s>%s is not a substitution between A, C, G and T", contig.c_str(),
                                         (long long)r.pos0 + 1, in_path, r.ref.c_str(), r.alts[a].c_str());
        }
        for (int s : by_name) {
            const std::vector<float>& af = r.af[(size_t)sample_col[(size_t)s]];
            for (size_t a = 0; a < n_alt && a < af.size(); ++a) {
                if (af[a] != af[a]) continue;
                vaf.push_back((double)af[a]);
                lnp.push_back(probs[a]);
                grp.push_back((by_sample ? s * kNSignatures : 0) + sig[a]);
            }
        }
    }
    if (n_entries) *n_entries = (int64_t)vaf.size();
    if (vaf.empty()) return ifail(VLR_ERR_INVALID_ARGUMENT, "unable to estimate TMB because no valid records were found in the given BCF/VCF");  // errors::Error::NoRecordsFound
    return vlr_launch_range_group_lse(device, (int64_t)vaf.size(), vaf.data(), lnp.data(), grp.data(), n_ranges, lo, hi, (by_sample ? n_samples : 1) * kNSignatures,
                                      kUploadPiece, out_cells);
}
