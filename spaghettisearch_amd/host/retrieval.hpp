// retrieval.hpp — host-side mirror of retrieval.Retrieve (retrieval/main_retrieve.go:15) above the C ABI.
//
// The query-time state lives on the GPU: DeviceIndex::load flattens inv[0]/inv[1] (already weighted by
// UpdateTermWeights), forw[4] magnitudes and forw[3] ranks once; Retrieve then parses the query on the
// host, makes ONE library call and maps the k winners into Rank_combined (util.go:25-36).
// Text normalisation (parser.Laundry: Porter2 stemming + stop words) and result decoration
// (get_metadata.go:79-235) are host-side Go in the reference and stay out of scope: `laundry` is a
// hook (default: lower-cased alphanumeric tokens), decoration fills DocHash/PageRank/FinalRank only.
// Quoted phrases (retrieval/phrase.go) are matched on the device from the positional part of the rows.
#pragma once
#include <cctype>
#include <chrono>
#include <condition_variable>
#include <fstream>
#include <functional>
#include <deque>
#include <future>
#include <mutex>
#include <thread>
#include <tuple>

#include "md5.hpp"
#include "ranking.hpp"

namespace retrieval {

struct Rank_combined {          // util.go:25-36 (decoration fields are left to the caller)
    std::string DocHash;
    double PageRank = 0;
    double FinalRank = 0;
    double TitleRank = 0, BodyRank = 0;   // diagnostics: the cosine-normalised parts
};

// Why a row is in a result (DeviceIndex::ExplainResults; no reference counterpart): the query's words, as md5-hex hashes in token
// order and each once, that the page holds in its title, in its body, and not at all; and the body position of the earliest matched
// word (the smallest position >= 0 over the query's words; none for a table without positions or a page matched in the title only).
struct ResultExplanation {
    std::vector<std::string> TitleWords, BodyWords, MissingWords;
    bool HasPosition = false;
    double FirstPosition = 0;
};

// "Did you mean" for one query token the index does not know (DeviceIndex::SuggestWords; no reference counterpart): the known words
// within the edit distance asked for, best first (distance, then frequency descending, then term id), as ss_lexicon_suggest orders them.
struct WordSuggestion {
    std::string Token;                       // the token as the tokeniser emits it
    std::vector<std::string> Words;          // suggested words of the vocabulary
    std::vector<int> Distances;              // byte edit distance of each (optimal string alignment)
    std::vector<uint32_t> Freqs;             // title + body list length of each, as the lexicon holds it
};

// One completion of what a user has typed (DeviceIndex::Complete; no reference counterpart): a word of the vocabulary that starts with
// the prefix and its frequency, rows ordered as ss_lexicon_complete orders them (frequency descending, then the word, then term id).
struct WordCompletion {
    std::string Word;
    uint32_t Freq = 0;                       // title + body list length, as the lexicon holds it
};

// Where a row's snippet should start (DeviceIndex::BestPassages; no reference counterpart, getSummary anchors at the first matched
// word): the window of `width` body positions that holds most of the query's distinct words, then most occurrences, then starts
// earliest.  Start / Last: the first and the last occurrence inside it (the caller cuts the cached words at [Start, Start + width));
// Words: the query's words found in the window, as md5-hex hashes in token order and each once; Distinct / Occurrences: the counts.
// HasPassage false (all else zero / empty): no positional postings, no such doc, or none of the words in the page's body text.
struct ResultPassage {
    bool HasPassage = false;
    double Start = 0, Last = 0;
    std::vector<std::string> Words;
    uint32_t Distinct = 0, Occurrences = 0;
};

// How close the query's words come in a row's body text (DeviceIndex::HitProximity; no reference counterpart): the smallest span of
// body positions that holds every query word the page has at all.  Start / End: its first and last occurrence; Words: the query's
// words the page has, as md5-hex hashes in token order and each once; Present: their number; Occurrences: the occurrences inside the
// span.  HasSpan false (all else zero / empty): no positional postings, no such doc, or none of the words in the page's body text.
struct ResultProximity {
    bool HasSpan = false;
    double Start = 0, End = 0;
    std::vector<std::string> Words;
    uint32_t Present = 0, Occurrences = 0;
};

// One page of a query's results re-ranked by term proximity (DeviceIndex::RetrieveBatchProximity; no reference counterpart).
// Scores[i] = w_rank * FinalRank + w_prox * bonus of Results[i]; Spans[i]: its ResultProximity.
struct ProximityPage {
    std::vector<Rank_combined> Results;
    std::vector<double> Scores;
    std::vector<ResultProximity> Spans;
};

// One page of a query's results re-ranked by a learned model (DeviceIndex::RetrieveBatchRanked; no reference counterpart).
// Scores[i] = the model's score of Results[i]'s feature row.
struct RankedPage {
    std::vector<Rank_combined> Results;
    std::vector<double> Scores;
};

// One page of a query's results with at most g rows per site (DeviceIndex::RetrieveBatchCollapsed; no reference counterpart).
// Same[i]: how many rows of the query's window are on the site of Results[i], the row itself included ("Same[i] - 1 more from this
// site"); Kept: how many rows the whole window keeps, i.e. how far paging can go.
struct CollapsedPage {
    std::vector<Rank_combined> Results;
    std::vector<uint32_t> Same;
    int Kept = 0;
};

// One page of a query's results without near-duplicate pages (DeviceIndex::RetrieveBatchDeduped; no reference counterpart).
// Similar[i]: how many rows of the query's window Results[i] stands for, itself included ("Similar[i] - 1 very similar results
// omitted"); Kept: how many rows the whole window keeps, i.e. how far paging can go.
struct DedupedPage {
    std::vector<Rank_combined> Results;
    std::vector<uint32_t> Similar;
    int Kept = 0;
};

// One range clause of DeviceIndex::RetrieveBatchFiltered: lo <= value <= hi on field 0 (Mod_date, unix seconds) or 1 (Page_size, bytes).
struct FieldRange {
    int32_t field = 0;
    int64_t lo = 0, hi = 0;
};

// One query's counts from DeviceIndex::FacetCounts (no reference counterpart): Total = the docs the query matches under its range
// clauses (and its "+word" / "-word" operators), Masks[name] = those of them in the named set of SetDocMasks, Buckets[b] = those whose
// field value lies in bucket b of the call.
struct FacetCount {
    uint32_t Total = 0;
    std::map<std::string, uint32_t> Masks;
    std::vector<uint32_t> Buckets;
};

// One query's sites from DeviceIndex::TopGroups (no reference counterpart): Total = the docs the query matches (FacetCount::Total),
// Groups = the distinct site keys among them, Ungrouped = the matches SetDocGroups does not name, Rows = page [first, first + m) of
// {site key, matches} by matches descending, equal counts by ascending key.
struct GroupPage {
    uint32_t Total = 0, Groups = 0, Ungrouped = 0;
    std::vector<std::pair<std::string, uint32_t>> Rows;
};

// One query's numbers from DeviceIndex::FieldStats (no reference counterpart): Total = the docs the query matches (FacetCount::Total);
// per asked field the smallest and largest value and the exact sum SumHi * 2^64 + SumLo (two's complement) over the Count matches that
// have a value, and the Missing ones that have none (SS_NO_FIELD_VALUE); Count + Missing = Total.  Count 0: Min INT64_MAX, Max INT64_MIN.
struct FieldStat {
    int64_t Min = INT64_MAX, Max = INT64_MIN;
    uint64_t SumLo = 0;
    int64_t SumHi = 0;
    uint32_t Count = 0, Missing = 0;
    double Mean() const { return Count ? ((double)SumHi * 18446744073709551616.0 + (double)SumLo) / (double)Count : 0.0; }   // for display
};
struct FieldStatsRow {
    uint32_t Total = 0;
    std::vector<FieldStat> Fields;
};
// One query's bins from DeviceIndex::FieldHistogram: Counts [n_bins], the matches below the first and at or above the last bin, those
// without a value, and Total = the sum of all of them = FacetCount::Total.
struct FieldHistogramRow {
    uint32_t Total = 0, Below = 0, Above = 0, Missing = 0;
    std::vector<uint32_t> Counts;
};

// One page of a query's results sorted by a doc field (DeviceIndex::SortByField; no reference counterpart).  Values[i]: the field's
// value of Results[i].
struct FieldSortedPage {
    std::vector<Rank_combined> Results;
    std::vector<int64_t> Values;
};

// One row of DeviceIndex::VectorSearch: a doc and its exact integer dot product with the query vector (no reference counterpart).
struct VectorHit {
    std::string DocHash;
    int32_t Score = 0;
};

// One page of a query's results re-ranked by vector score (DeviceIndex::RerankByVector, RerankByMaxSim).  Scores[i]: the score of Results[i],
// SS_NO_VEC_SCORE for a row whose doc hash the index does not hold.
struct VectorRerankedPage {
    std::vector<Rank_combined> Results;
    std::vector<int32_t> Scores;
};

// One page of a query's results diversified (DeviceIndex::DiversifyByVector).  Rel[i]: the relevance Results[i] was chosen with (its
// vector score, or minus its window position when the call was by rank); Sim[i]: its largest similarity to the rows chosen before it,
// SS_NO_VEC_SCORE for the first row.  Both SS_NO_VEC_SCORE for a row whose doc hash the index does not hold.
struct DiversifiedPage {
    std::vector<Rank_combined> Results;
    std::vector<int32_t> Rel, Sim;
};

// How DeviceIndex::HybridSearch fuses the lexical and the vector ranking (ss_fuse_params): reciprocal rank fusion,
// w_lex / (rrf_c + lexical rank) + w_vec / (rrf_c + vector rank), or (weighted) w_lex * FinalRank + w_vec * vector score.
struct HybridParams {
    bool weighted = false;
    int rrf_c = 60;
    double w_lex = 1.0, w_vec = 1.0;
};

// One page of a query's fused results (DeviceIndex::HybridSearch; no reference counterpart).  Per row its fused score, its vector
// score and its 1-based rank in the lexical and in the vector window (0: the window does not hold it); Union: the distinct docs of
// both windows, the length of the fused ranking.
struct HybridPage {
    std::vector<Rank_combined> Results;
    std::vector<double> Scores;
    std::vector<int32_t> VecScores;
    std::vector<int> LexRanks, VecRanks;
    int Union = 0;
};

// util.go:151-160: quoted phrases `".*?"`
inline std::vector<std::string> getPhrase(const std::string& s) {
    std::vector<std::string> out;
    size_t i = 0;
    while ((i = s.find('"', i)) != std::string::npos) {
        const size_t j = s.find('"', i + 1);
        if (j == std::string::npos) break;
        out.push_back(s.substr(i + 1, j - i - 1));
        i = j + 1;
    }
    return out;
}

// parser.go:177-193 without stemming / stop words (those stay host-side Go)
inline std::vector<std::string> defaultLaundry(const std::string& s) {
    std::vector<std::string> out;
    std::string cur;
    for (unsigned char c : s) {
        if (std::isalnum(c)) cur += (char)std::tolower(c);
        else if (!cur.empty()) { out.push_back(cur); cur.clear(); }
    }
    if (!cur.empty()) out.push_back(cur);
    return out;
}

// Query operators (no reference counterpart; DeviceIndex::SetQueryOperators, default off).  Outside quoted phrases (the `".*?"`
// pairs of getPhrase), a whitespace-separated token whose first character is '+' or '-' and whose second is one that `laundry`
// keeps is an operator token: every word it launders to is REQUIRED ('+': each result must contain it) or EXCLUDED ('-': no result
// may).  `query` is the string the scorer tokenises: '+' tokens stay in it (their words are scored and counted in query_len, as any
// word), '-' tokens are taken out.  "e-mail", a lone "-", "--x" and everything between quotes are no operators.
struct QueryOperators {
    std::string query;
    std::vector<std::string> required, excluded;
};
inline QueryOperators parseQueryOperators(const std::string& query,
                                          const std::function<std::vector<std::string>(const std::string&)>& laundry = defaultLaundry) {
    QueryOperators out;
    std::vector<size_t> quotes;                          // the quotes that pair up as getPhrase's matches do: 0-1, 2-3, ...
    for (size_t i = 0; i < query.size(); i++)
        if (query[i] == '"') quotes.push_back(i);
    if (quotes.size() % 2) quotes.pop_back();
    size_t qi = 0, i = 0;
    while (i < query.size()) {
        if (qi < quotes.size() && i == quotes[qi]) {     // a quoted phrase: copied as it is
            out.query.append(query, i, quotes[qi + 1] + 1 - i);
            i = quotes[qi + 1] + 1;
            qi += 2;
            continue;
        }
        if (std::isspace((unsigned char)query[i])) { out.query += query[i++]; continue; }
        size_t j = i;                                    // a token: up to whitespace or the next phrase
        while (j < query.size() && !std::isspace((unsigned char)query[j]) && !(qi < quotes.size() && j == quotes[qi])) j++;
        const std::string tok = query.substr(i, j - i);
        const bool op = tok.size() > 1 && (tok[0] == '+' || tok[0] == '-') && !laundry(tok.substr(1, 1)).empty();
        if (op) {
            std::vector<std::string>& dst = tok[0] == '+' ? out.required : out.excluded;
            for (auto& w : laundry(tok.substr(1))) dst.push_back(w);
        }
        if (!op || tok[0] == '+') out.query += tok;
        i = j;
    }
    return out;
}

// Prefix tokens (no reference counterpart; DeviceIndex::SetPrefixQueries, default off).  Outside quoted phrases (paired as above), a
// whitespace-separated token that ends in '*' with at least one byte before the star is a prefix token: it is taken out of `query`,
// the string the tokeniser sees, and its bytes without the star, ASCII lower-cased and NOT stemmed, go to `prefixes` in the order they
// stand.  Only the trailing star counts ("a*b" is a plain token, "*" alone too).  skip_operators (the strings of SetQueryOperators):
// a token parseQueryOperators reads as "+word" / "-word" is no prefix token, its star is left to the tokeniser as before.
struct PrefixTokens {
    std::string query;
    std::vector<std::string> prefixes;
};
inline PrefixTokens parsePrefixTokens(const std::string& query, bool skip_operators,
                                      const std::function<std::vector<std::string>(const std::string&)>& laundry = defaultLaundry) {
    PrefixTokens out;
    std::vector<size_t> quotes;
    for (size_t i = 0; i < query.size(); i++)
        if (query[i] == '"') quotes.push_back(i);
    if (quotes.size() % 2) quotes.pop_back();
    size_t qi = 0, i = 0;
    while (i < query.size()) {
        if (qi < quotes.size() && i == quotes[qi]) {     // a quoted phrase: copied as it is
            out.query.append(query, i, quotes[qi + 1] + 1 - i);
            i = quotes[qi + 1] + 1;
            qi += 2;
            continue;
        }
        if (std::isspace((unsigned char)query[i])) { out.query += query[i++]; continue; }
        size_t j = i;
        while (j < query.size() && !std::isspace((unsigned char)query[j]) && !(qi < quotes.size() && j == quotes[qi])) j++;
        const std::string tok = query.substr(i, j - i);
        const bool op = skip_operators && tok.size() > 1 && (tok[0] == '+' || tok[0] == '-') && !laundry(tok.substr(1, 1)).empty();
        if (!op && tok.size() > 1 && tok.back() == '*') {
            std::string pre = tok.substr(0, tok.size() - 1);
            for (auto& c : pre)
                if (c >= 'A' && c <= 'Z') c = (char)(c - 'A' + 'a');
            out.prefixes.push_back(pre);
        } else {
            out.query += tok;
        }
        i = j;
    }
    return out;
}

// computeTopicProbs, retrieval/main_retrieve.go:106-159 — DISABLED in the reference (the call at :43 is commented out and
// :87 passes a nil map, so sqd = 0); restated so that the PageRank blend of get_metadata.go:39-42,69 can be switched on.
//   queryTokenised: md5-hex word hashes as Retrieve makes them (:33-36);
//   metadata = forw[5] rows {numPages, wordCount} (:110); inv[2][word] = map[category]frequency (:120-124) — a word
//   that is not in inv[2] throws db::KeyNotFound, where the reference panics (:120-121);
//   as_written = true reproduces `var probs float64` (:142): the product starts at 0, every probability is 0;
//   as_written = false starts it at 1 (multinomial naive Bayes with max-likelihood estimates, uniform prior 1/K, :148).
inline std::map<std::string, double> computeTopicProbs(db::Context& ctx, std::vector<db::DB*>& inv, std::vector<db::DB*>& forw,
                                                       const std::vector<std::string>& queryTokenised, bool as_written) {
    std::map<std::string, std::map<std::string, double>> metadata;                       // :110
    for (auto& kv : forw[5]->Iterate(ctx)) metadata[kv.first] = jsonmini::parse_map_f64(kv.second);
    std::map<std::string, std::vector<double>> topicTF;                                  // :118
    for (auto& tok : queryTokenised) {
        const std::map<std::string, double> topicFreq = jsonmini::parse_map_f64(inv[2]->Get(ctx, tok));   // :120-124 (throws = panic)
        for (auto& tf : topicFreq) topicTF[tf.first].push_back(tf.second);               // :126-134
    }
    std::map<std::string, double> topicProbs;                                            // :137
    for (auto& md : metadata) {
        auto it = topicTF.find(md.first);
        if (it != topicTF.end()) {
            double probs = as_written ? 0.0 : 1.0;                                       // :142
            auto wc = md.second.find("wordCount");
            const double wordCount = wc == md.second.end() ? 0.0 : wc->second;           // missing key reads as 0 in Go
            for (double tf : it->second) probs *= (tf / wordCount);                      // :143-145
            topicProbs[md.first] = probs / (double)metadata.size();                      // :148
        } else {
            topicProbs[md.first] = 0;                                                    // :150
        }
    }
    return topicProbs;
}

// The query-time tables flattened to dense ids: what DeviceIndex::load decodes from the JSON rows and
// uploads, and what a snapshot file holds — so that a server start does not pay the reference's dominant load cost
// (json.Unmarshal of every posting map, database/noschema_schema.go:125-260) again.
//   file = "SSNAP002" | u64 n_docs, n_terms, K | doc names, term names, categories (u32 length + bytes each) |
//          per table (title, body): u64 P, u64 n_pos | term_ptr u64[T+1] | post_doc u32[P] | post_w f32[P] |
//          pos_ptr u64[P+1] | pos f32[n_pos] | mag f64[n_docs]   |   prior f64[K][n_docs]
struct FlatTable {
    std::vector<uint64_t> term_ptr, pos_ptr;
    std::vector<uint32_t> post_doc;
    std::vector<float> post_w, pos;
    std::vector<double> mag;
};
struct FlatCorpus {
    std::vector<std::string> doc_names, term_names, categories;
    FlatTable title, body;
    std::vector<double> prior;       // [K][n_docs]

    template <typename T>
    static void put(std::ostream& f, const std::vector<T>& v) { f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T))); }
    template <typename T>
    static void get(std::istream& f, std::vector<T>& v, size_t n) {
        v.resize(n);
        f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(n * sizeof(T)));
        if (!f) throw std::runtime_error("snapshot: file truncated");
    }
    static void put_u64(std::ostream& f, uint64_t x) { f.write(reinterpret_cast<const char*>(&x), 8); }
    static uint64_t get_u64(std::istream& f) {
        uint64_t x = 0;
        f.read(reinterpret_cast<char*>(&x), 8);
        if (!f) throw std::runtime_error("snapshot: file truncated");
        return x;
    }
    static void put_names(std::ostream& f, const std::vector<std::string>& v) {
        for (auto& s : v) { const uint32_t n = (uint32_t)s.size(); f.write(reinterpret_cast<const char*>(&n), 4); f.write(s.data(), n); }
    }
    static void get_names(std::istream& f, std::vector<std::string>& v, size_t count) {
        v.resize(count);
        for (auto& s : v) {
            uint32_t n = 0;
            f.read(reinterpret_cast<char*>(&n), 4);
            if (!f || n > (1u << 20)) throw std::runtime_error("snapshot: bad name record");
            s.resize(n);
            f.read(&s[0], n);
            if (!f) throw std::runtime_error("snapshot: file truncated");
        }
    }
    void save(const std::string& path) const {
        std::ofstream f(path, std::ios::binary | std::ios::trunc);
        if (!f) throw std::runtime_error("snapshot: cannot open " + path + " for writing");
        f.write("SSNAP002", 8);
        put_u64(f, doc_names.size());
        put_u64(f, term_names.size());
        put_u64(f, categories.size());
        put_names(f, doc_names);
        put_names(f, term_names);
        put_names(f, categories);
        for (const FlatTable* t : {&title, &body}) {
            put_u64(f, t->post_doc.size());
            put_u64(f, t->pos.size());
            put(f, t->term_ptr); put(f, t->post_doc); put(f, t->post_w); put(f, t->pos_ptr); put(f, t->pos); put(f, t->mag);
        }
        put(f, prior);
        if (!f) throw std::runtime_error("snapshot: write to " + path + " failed");
    }
    void load(const std::string& path) {
        std::ifstream f(path, std::ios::binary);
        if (!f) throw std::runtime_error("snapshot: cannot open " + path);
        char magic[8];
        f.read(magic, 8);
        if (!f || std::string(magic, 8) != "SSNAP002") throw std::runtime_error("snapshot: " + path + " is not an SSNAP002 file");
        const uint64_t n = get_u64(f), T = get_u64(f), K = get_u64(f);
        get_names(f, doc_names, n);
        get_names(f, term_names, T);
        get_names(f, categories, K);
        for (FlatTable* t : {&title, &body}) {
            const uint64_t P = get_u64(f), np = get_u64(f);
            get(f, t->term_ptr, T + 1); get(f, t->post_doc, P); get(f, t->post_w, P); get(f, t->pos_ptr, P + 1); get(f, t->pos, np); get(f, t->mag, n);
            if (t->term_ptr[T] != P || t->pos_ptr[P] != np) throw std::runtime_error("snapshot: inconsistent table sizes");
        }
        get(f, prior, K * n);
    }
};

// What the indexer writes for one page (indexer/indexer.go:23-348): its own postings in inv[0] / inv[1] (setInverted
// :350-408, listPos = [normTF, positions...]), the anchor words it puts into the TITLE rows of its children (:236-290,
// positions -100) and its forw[2] row.  `before` = what checkAndUpdate (:420-641) removes, `after` = what the re-index adds.
struct PageIndexInfo {
    std::string docHash;
    std::map<std::string, std::vector<float>> title, body;                           // wordHash -> listPos
    std::map<std::string, std::map<std::string, std::vector<float>>> anchors;        // childHash -> wordHash -> listPos
    std::vector<std::string> children;                                               // forw[2][docHash]
};

class DeviceIndex {
public:
    spaghetti::DenseIds docs, terms;
    FlatCorpus flat;                 // kept for save_snapshot (host memory; drop with flat = {} when not needed)
    ss_index* title = nullptr;
    ss_index* body = nullptr;
    ss_scorer* scorer = nullptr;
    std::vector<std::string> categories;
    std::function<std::vector<std::string>(const std::string&)> laundry = defaultLaundry;
    bool mags_resident = false;      // squared magnitudes resident on the device: deltas keep them up to date
    bool flat_stale = false;         // deltas were applied since `flat` was filled
    // Named doc allow-lists (no reference counterpart): "search within a category" (TopicTeleportSets' doc set of an ODP
    // category used as a result restriction), "hide these pages".  Kept by doc hash: every scorer this index creates (upload,
    // ApplyDelta) gets them again, with the ids as they stand then.
    std::map<std::string, std::vector<std::string>> mask_sets;
    std::map<std::string, int32_t> mask_index;      // name -> the scorer's mask id
    bool query_operators = false;                   // SetQueryOperators: "+word" / "-word" in RetrieveBatch's query strings
    int prefix_expansions = 0;                      // SetPrefixQueries: "word*" in query strings stands for its most frequent completions (0: off)
    bool similar_pages = false;                     // SetSimilarPages: the body table keeps its doc-major view (8 B per posting + 8 B per doc)
    bool doc_view_built = false;                    // the body table holds a view that this object built and nothing has freed since
    // Site keys for collapsed result pages (SetDocGroups): doc hash -> key string, kept by hash like the allow-lists and registered
    // again on every scorer this index creates.  has_doc_groups: SetDocGroups was called (an empty map is a table of SS_NO_GROUP).
    std::map<std::string, std::string> doc_group_keys;
    std::vector<std::string> doc_group_names;       // the key behind every group number of the registered table (register_groups)
    bool has_doc_groups = false;
    // Doc fields (SetDocFields): doc hash -> {Mod_date as unix seconds, Page_size} (retrieval/util.go:28-29), kept by hash like the site
    // keys and registered again on every scorer this index creates.
    std::map<std::string, std::pair<int64_t, int64_t>> doc_field_values;
    bool has_doc_fields = false;
    // Doc vectors (SetDocVectors): doc hash -> int8 embedding of doc_vector_dim values, kept by hash like the fields and registered
    // again on every scorer this index creates.
    std::map<std::string, std::vector<int8_t>> doc_vectors;
    int doc_vector_dim = 0;
    // Vector lists (SetVectorLists): the centroids [n_vector_lists][doc_vector_dim], kept and assigned again on every scorer the index
    // creates, as the vectors are; a later SetDocVectors clears them.
    std::vector<int8_t> list_centroids;
    int n_vector_lists = 0;
    // Doc tokens (SetDocTokens): doc hash -> its token vectors, each of doc_token_dim int8 values, kept by hash and registered again on
    // every scorer this index creates, as the vectors are; independent of them.
    std::map<std::string, std::vector<std::vector<int8_t>>> doc_tokens;
    int doc_token_dim = 0;
    int near_dup_slots = 0;                         // SetNearDuplicates: the body table keeps MinHash signatures of this many slots (4 B each per doc)
    bool signatures_built = false;                  // the body table holds signatures that this object built and nothing has freed since
    // Term lexicon (SetLexicon): the word of every resident term id, on the device (ss_lexicon) and here for the answers; lex_freq
    // = title + body list length per term.  upload() drops it (the term ids are new): call SetLexicon again after load().
    ss_lexicon* lexicon = nullptr;
    std::vector<std::string> lex_words;
    std::vector<uint32_t> lex_freq;
    std::vector<bool> lex_known;                    // forw[0] held the term's hash when its word was read
    // Learned ranking (SetRankModel): a tree ensemble over the SS_RANK_N_FEATURES columns of ss_hit_features.  It reads no table of
    // the index, so upload() and ApplyDelta leave it alone.
    ss_rank_model* rank_model = nullptr;

    ~DeviceIndex() {
        if (rank_model) ss_rank_model_destroy(rank_model);
        if (lexicon) ss_lexicon_destroy(lexicon);
        if (scorer) ss_scorer_destroy(scorer);
        if (title) ss_index_destroy(title);
        if (body) ss_index_destroy(body);
    }

    void load(db::Context& ctx, std::vector<db::DB*>& forw, std::vector<db::DB*>& inv) {
        using namespace spaghetti;
        const std::vector<db::KV> ranks = forw[3]->Iterate(ctx);
        std::vector<std::map<std::string, std::vector<float>>> trow, brow;
        std::vector<std::string> all_docs, all_terms;
        for (auto& kv : ranks) all_docs.push_back(kv.first);
        const std::vector<db::KV> tcomp = inv[0]->Iterate(ctx), bcomp = inv[1]->Iterate(ctx);
        for (auto& kv : tcomp) { all_terms.push_back(kv.first); trow.push_back(jsonmini::parse_map_f32list(kv.second)); }
        for (auto& kv : bcomp) { all_terms.push_back(kv.first); brow.push_back(jsonmini::parse_map_f32list(kv.second)); }
        for (auto& r : trow) for (auto& kv : r) all_docs.push_back(kv.first);
        for (auto& r : brow) for (auto& kv : r) all_docs.push_back(kv.first);
        docs.build(all_docs.begin(), all_docs.end());
        terms.build(all_terms.begin(), all_terms.end());
        const size_t n = docs.name.size(), T = terms.name.size();
        auto flatten = [&](const std::vector<db::KV>& comp, std::vector<std::map<std::string, std::vector<float>>>& rows,
                           std::vector<uint64_t>& ptr, std::vector<uint32_t>& doc, std::vector<float>& w,
                           std::vector<uint64_t>& pos_ptr, std::vector<float>& pos) {
            std::vector<const std::map<std::string, std::vector<float>>*> by_term(T, nullptr);
            for (size_t i = 0; i < comp.size(); i++) by_term[terms.id[comp[i].first]] = &rows[i];
            ptr.assign(T + 1, 0);
            for (size_t t = 0; t < T; t++) ptr[t + 1] = ptr[t] + (by_term[t] ? by_term[t]->size() : 0);
            doc.resize(ptr[T]);
            w.resize(ptr[T]);
            pos_ptr.assign(1, 0);
            pos.clear();
            for (size_t t = 0; t < T; t++) {
                if (!by_term[t]) continue;
                uint64_t j = ptr[t];
                for (auto& kv : *by_term[t]) {
                    doc[j] = docs.id[kv.first];
                    w[j] = kv.second.at(0);                                            // first entry = norm_tf*idf (main_retrieve.go:227,236)
                    pos.insert(pos.end(), kv.second.begin() + 1, kv.second.end());     // listPos[1:] = positions (phrase.go:144-146)
                    pos_ptr.push_back(pos.size());
                    j++;
                }
            }
        };
        flatten(tcomp, trow, flat.title.term_ptr, flat.title.post_doc, flat.title.post_w, flat.title.pos_ptr, flat.title.pos);
        flatten(bcomp, brow, flat.body.term_ptr, flat.body.post_doc, flat.body.post_w, flat.body.pos_ptr, flat.body.pos);
        // forw[4]: a missing "title"/"body" key reads as 0 (get_metadata.go:57-58, Q8)
        flat.title.mag.assign(n, 0.0);
        flat.body.mag.assign(n, 0.0);
        for (auto& kv : forw[4]->Iterate(ctx)) {
            auto it = docs.id.find(kv.first);
            if (it == docs.id.end()) continue;
            auto m = jsonmini::parse_map_f64(kv.second);
            flat.title.mag[it->second] = m.count("title") ? m["title"] : 0.0;
            flat.body.mag[it->second] = m.count("body") ? m["body"] : 0.0;
        }
        // forw[3]: ranks per category, for the PageRank blend (get_metadata.go:31-42)
        std::vector<std::string> cat;
        for (auto& kv : ranks) for (auto& c : jsonmini::parse_map_f64(kv.second)) cat.push_back(c.first);
        std::sort(cat.begin(), cat.end());
        cat.erase(std::unique(cat.begin(), cat.end()), cat.end());
        flat.categories = cat;
        const size_t K = cat.size();
        flat.prior.assign(K * n, 0.0);
        for (auto& kv : ranks) {
            const uint32_t d = docs.id[kv.first];
            for (auto& c : jsonmini::parse_map_f64(kv.second)) {
                const size_t k = std::lower_bound(cat.begin(), cat.end(), c.first) - cat.begin();
                flat.prior[k * n + d] = c.second;
            }
        }
        flat.doc_names = docs.name;
        flat.term_names = terms.name;
        upload();
    }

    // flat arrays -> device state (ss_index x2, positions, magnitudes, scorer, prior)
    void upload() {
        using namespace spaghetti;
        if (scorer) { ss_scorer_destroy(scorer); scorer = nullptr; }
        if (title) { ss_index_destroy(title); title = nullptr; }
        if (body) { ss_index_destroy(body); body = nullptr; }
        drop_lexicon();
        mags_resident = flat_stale = doc_view_built = signatures_built = false;
        const size_t n = flat.doc_names.size(), T = flat.term_names.size();
        check(ss_index_create(default_ctx(), n, T, flat.title.term_ptr.data(), flat.title.post_doc.data(), flat.title.post_w.data(), &title), "ss_index_create(title)");
        check(ss_index_create(default_ctx(), n, T, flat.body.term_ptr.data(), flat.body.post_doc.data(), flat.body.post_w.data(), &body), "ss_index_create(body)");
        check(ss_index_set_positions(title, flat.title.pos_ptr.data(), flat.title.pos.data()), "ss_index_set_positions(title)");
        check(ss_index_set_positions(body, flat.body.pos_ptr.data(), flat.body.pos.data()), "ss_index_set_positions(body)");
        check(ss_index_set_weighted(title, flat.title.mag.data()), "ss_index_set_weighted(title)");
        check(ss_index_set_weighted(body, flat.body.mag.data()), "ss_index_set_weighted(body)");
        check(ss_scorer_create(default_ctx(), title, body, &scorer), "ss_scorer_create");
        categories = flat.categories;
        const size_t K = categories.size();
        if (K > 0 && K <= SS_MAX_TOPICS) check(ss_scorer_set_prior(scorer, (int32_t)K, flat.prior.data()), "ss_scorer_set_prior");
        register_masks();
        register_groups();
        register_fields();
        register_vectors();
        register_tokens();
        build_doc_view();
        build_signatures();
    }

    // Similar pages (no reference counterpart; default off: nothing is built and memory is as it was).  On, the body table's
    // doc-major view (ss_index_build_doc_view) is built now and again after every upload / ApplyDelta that re-creates the scorer
    // (a delta frees the view with the postings it was made from); off, the view is freed.
    void SetSimilarPages(bool on) {
        similar_pages = on;
        if (on) build_doc_view();
        else if (body && doc_view_built) { doc_view_built = false; spaghetti::check(ss_index_drop_doc_view(body), "ss_index_drop_doc_view(body)"); }
    }
    void build_doc_view() {
        if (!similar_pages || !body) return;
        doc_view_built = false;                                 // (a failing build leaves the table without a view)
        spaghetti::check(ss_index_build_doc_view(body), "ss_index_build_doc_view(body)");
        doc_view_built = true;
    }
    bool HasDocView() const { return doc_view_built; }
    // Near-duplicate results (no reference counterpart; default off).  n_slots = 4, 8, .., 32: the body table gets a MinHash
    // signature per doc (ss_index_build_signatures), built now and again after every upload / ApplyDelta (a delta frees the
    // signatures with the postings they were made from); 0 frees them.  The signatures are made from the body table's doc view:
    // a view built only for them (SetSimilarPages off) is freed again once they exist.
    void SetNearDuplicates(int n_slots) {
        if (n_slots == 0) {
            near_dup_slots = 0;
            if (body && signatures_built) { signatures_built = false; spaghetti::check(ss_index_drop_signatures(body), "ss_index_drop_signatures(body)"); }
            return;
        }
        const int before = near_dup_slots;
        near_dup_slots = n_slots;
        try { build_signatures(); } catch (...) { near_dup_slots = before; throw; }
    }
    void build_signatures() {
        if (!near_dup_slots || !body) return;
        if (!doc_view_built) spaghetti::check(ss_index_build_doc_view(body), "ss_index_build_doc_view(body)");
        const int32_t rc = ss_index_build_signatures(body, near_dup_slots);
        if (rc == SS_OK || (rc != SS_ERR_INVALID && rc != SS_ERR_UNSUPPORTED)) signatures_built = rc == SS_OK;   // (a refused n_slots leaves what exists)
        if (!doc_view_built) (void)ss_index_drop_doc_view(body);
        spaghetti::check(rc, "ss_index_build_signatures(body)");
    }
    int NearDuplicateSlots() const { return signatures_built ? near_dup_slots : 0; }
    // the m heaviest body words of a page (word hashes; weight descending, then dense term id), empty for an unknown hash
    std::vector<std::string> DocTopTerms(const std::string& docHash, int m = 5) {
        using namespace spaghetti;
        auto it = docs.id.find(docHash);
        if (it == docs.id.end()) return {};
        std::vector<uint32_t> t((size_t)std::max(m, 1));
        int32_t n = 0;
        check(ss_index_doc_top_terms(body, 1, &it->second, m, t.data(), nullptr, &n), "ss_index_doc_top_terms");
        return term_hashes(t.data(), n);
    }
    // "Similar pages" of a result card: the page's m heaviest body words as a new query (ss_similar_topk), the page itself left
    // out; the same Rank_combined rows Retrieve returns.  mask: a set of SetDocMasks, "" = the whole index.  An unknown hash
    // gives an empty result.  Needs SetSimilarPages(true).
    std::vector<Rank_combined> SimilarPages(const std::string& docHash, const std::string& mask, int k = 50, int m = 5) {
        using namespace spaghetti;
        if (!similar_pages) throw std::runtime_error("SimilarPages: switched off (SetSimilarPages)");
        int32_t mask_id = -1;
        if (!mask.empty()) {
            auto mi = mask_index.find(mask);
            if (mi == mask_index.end()) throw std::runtime_error("SimilarPages: no doc mask named '" + mask + "' (SetDocMasks)");
            mask_id = mi->second;
        }
        auto it = docs.id.find(docHash);
        if (it == docs.id.end()) return {};
        std::vector<ss_hit> hits((size_t)std::max(k, 1));
        std::vector<int32_t> n_hits(1);
        check(ss_similar_topk(scorer, 1, &it->second, m, nullptr, mask.empty() ? nullptr : &mask_id, k, hits.data(), n_hits.data()), "ss_similar_topk");
        return to_ranks(1, k, hits, n_hits)[0];
    }
    std::vector<Rank_combined> SimilarPages(const std::string& docHash, int k = 50, int m = 5) { return SimilarPages(docHash, std::string(), k, m); }
    // "Related searches" of a result list: the m words (hashes, best first) that the k_fb best pages of `query` have in common
    // among their m_doc heaviest body words and that the user did not type (ss_related_terms).  The query is tokenised as Retrieve
    // does; quoted phrases and '+' / '-' operators are not interpreted (the phrase words leave the query, operator tokens are plain
    // words).  Needs SetSimilarPages(true): the body view must exist.
    std::vector<std::string> RelatedTerms(const std::string& query, int m = 10, int k_fb = 10, int m_doc = 5) {
        using namespace spaghetti;
        if (!similar_pages) throw std::runtime_error("RelatedTerms: switched off (SetSimilarPages)");
        const Tokenised t = tokenise({query}, nullptr, false);
        std::vector<uint32_t> ids((size_t)std::max(m, 1));
        int32_t n = 0;
        check(ss_related_terms(scorer, 1, t.q_ptr.data(), t.q_terms.data(), nullptr, nullptr, nullptr, k_fb, m_doc, m, ids.data(), nullptr, &n),
              "ss_related_terms");
        return term_hashes(ids.data(), n);
    }
    // Per row of `results` — the Rank_combined rows Retrieve / RetrieveBatch returned for `query` — which of the query's words matched
    // where (ss_explain_hits).  The query is tokenised as Retrieve does; the words of quoted phrases count as tokens, behind the
    // others.  With SetQueryOperators(true) the string is read as RetrieveBatch reads it: '-' tokens leave the query, '+' tokens are
    // plain words.  A row whose DocHash the index does not hold lacks every word.  Changes nothing unless called.
    std::vector<ResultExplanation> ExplainResults(const std::string& query, const std::vector<Rank_combined>& results) {
        using namespace spaghetti;
        const std::vector<std::string> hashed = query_word_hashes(query);
        std::vector<ResultExplanation> out(results.size());
        if (results.empty()) return out;
        auto add_once = [](std::vector<std::string>& v, const std::string& x) {
            if (std::find(v.begin(), v.end(), x) == v.end()) v.push_back(x);
        };
        const size_t k = results.size(), T = hashed.size();
        if (T == 0) return out;
        if (k > (size_t)SS_MAX_TOPK || T > (size_t)SS_MAX_QUERY_TERMS) throw std::runtime_error("ExplainResults: too many rows or query words");
        std::vector<uint32_t> q_ptr{0, (uint32_t)T}, q_terms;
        for (auto& h : hashed) {
            auto it = terms.id.find(h);
            q_terms.push_back(it == terms.id.end() ? SS_UNKNOWN_TERM : it->second);
        }
        std::vector<ss_hit> hits(k);
        for (size_t j = 0; j < k; j++) {
            auto it = docs.id.find(results[j].DocHash);
            hits[j] = ss_hit{};
            hits[j].doc = it == docs.id.end() ? 0xFFFFFFFFu : it->second;      // no such doc: no postings
        }
        const int32_t n_hits = (int32_t)k;
        std::vector<ss_term_match> m(k * T);
        check(ss_explain_hits(scorer, 1, q_ptr.data(), q_terms.data(), (int32_t)k, hits.data(), &n_hits, (int32_t)T, m.data()), "ss_explain_hits");
        for (size_t j = 0; j < k; j++)
            for (size_t i = 0; i < T; i++) {
                const ss_term_match& e = m[j * T + i];
                if (e.flags & 1u) add_once(out[j].TitleWords, hashed[i]);
                if (e.flags & 2u) add_once(out[j].BodyWords, hashed[i]);
                if (!(e.flags & 3u)) add_once(out[j].MissingWords, hashed[i]);
                if ((e.flags & 4u) && (!out[j].HasPosition || (double)e.body_pos < out[j].FirstPosition)) {
                    out[j].HasPosition = true;
                    out[j].FirstPosition = (double)e.body_pos;
                }
            }
        return out;
    }
    // The query's word hashes in token order, as ExplainResults and BestPassages read a query string: tokenised as Retrieve does; the
    // words of quoted phrases count as tokens, behind the others.  With SetQueryOperators(true) the string is read as RetrieveBatch
    // reads it: '-' tokens leave the query, '+' tokens are plain words.
    std::vector<std::string> query_word_hashes(const std::string& query) const {
        std::vector<std::string> hashed;
        for (auto& w : query_words(query)) hashed.push_back(md5::hex(w));
        return hashed;
    }
    // ... and the words themselves, before hashing (SuggestWords)
    std::vector<std::string> query_words(const std::string& query) const {
        std::string text = query_operators ? parseQueryOperators(query, laundry).query : query;
        const std::vector<std::string> phrases = getPhrase(text);      // main_retrieve.go:17-36, as tokenise()
        for (auto& ph : phrases) {
            const size_t pos = text.find("\"" + ph + "\"");
            if (pos != std::string::npos) text.erase(pos, ph.size() + 2);
        }
        std::string joined;
        for (auto& ph : phrases) joined += ph + " ";
        std::vector<std::string> words = laundry(text);
        for (auto& w : laundry(joined)) words.push_back(w);
        return words;
    }
    // Term lexicon (ss_lexicon; the reference's /wordlist/{pre}, cmd/server/server.go:54-85, and "did you mean").  forw0 = forw[0],
    // wordHash -> word: read for every resident term id; a term whose hash is missing there gets the empty word and freq 0.  freq =
    // title list length + body list length, saturated at 2^32 - 1.  Changes nothing unless called.
    void SetLexicon(db::Context& ctx, db::DB* forw0) {
        if (!title || !body) throw std::runtime_error("SetLexicon: the index is not loaded");
        lex_words.assign(terms.name.size(), std::string());
        lex_known.assign(terms.name.size(), false);
        for (size_t t = 0; t < terms.name.size(); t++)
            if (forw0->Has(ctx, terms.name[t])) { lex_words[t] = forw0->Get(ctx, terms.name[t]); lex_known[t] = true; }
        build_lexicon(lex_known);
    }
    bool HasLexicon() const { return lexicon != nullptr; }
    void drop_lexicon() {
        if (lexicon) { ss_lexicon_destroy(lexicon); lexicon = nullptr; }
        lex_words.clear();
        lex_freq.clear();
        lex_known.clear();
    }
    // title + body list length of every term as the resident tables stand; 0 for a term forw[0] does not know
    void read_lex_freq(const std::vector<bool>& known) {
        using namespace spaghetti;
        const size_t T = terms.name.size();
        std::vector<uint64_t> tp(T + 1), bp(T + 1);
        check(ss_index_read(title, tp.data(), nullptr, nullptr), "ss_index_read(title)");
        check(ss_index_read(body, bp.data(), nullptr, nullptr), "ss_index_read(body)");
        lex_freq.assign(T, 0u);
        for (size_t t = 0; t < T; t++) {
            const uint64_t f = (tp[t + 1] - tp[t]) + (bp[t + 1] - bp[t]);
            lex_freq[t] = !known[t] ? 0u : f > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)f;
        }
    }
    void build_lexicon(const std::vector<bool>& known) {
        using namespace spaghetti;
        if (lexicon) { ss_lexicon_destroy(lexicon); lexicon = nullptr; }
        read_lex_freq(known);
        std::vector<uint64_t> ptr(lex_words.size() + 1, 0);
        std::string bytes;
        for (size_t t = 0; t < lex_words.size(); t++) {
            bytes += lex_words[t];
            ptr[t + 1] = bytes.size();
        }
        check(ss_lexicon_create(default_ctx(), lex_words.size(), ptr.data(), reinterpret_cast<const uint8_t*>(bytes.data()), lex_freq.data(), &lexicon),
              "ss_lexicon_create");
    }
    // after a delta: new term ids -> the lexicon is made again (their words from forw[0]); otherwise only the frequencies follow
    void refresh_lexicon(db::Context& ctx, db::DB* forw0, size_t t_before) {
        if (!lexicon) return;
        if (terms.name.size() != t_before) {
            lex_words.resize(terms.name.size());
            lex_known.resize(terms.name.size(), false);
            for (size_t t = t_before; t < terms.name.size(); t++)
                if (forw0->Has(ctx, terms.name[t])) { lex_words[t] = forw0->Get(ctx, terms.name[t]); lex_known[t] = true; }
            build_lexicon(lex_known);
        } else {
            read_lex_freq(lex_known);
            spaghetti::check(ss_lexicon_set_freq(lexicon, lex_freq.data()), "ss_lexicon_set_freq");
        }
    }
    // The route's answer, one page of it: the words that start with `pre`, sorted as the reference sorts them (bytes, a proper prefix
    // first), entries first .. first + k.  Terms without a word in forw[0] hold the empty word and are listed under the empty prefix only.
    std::vector<std::string> WordList(const std::string& pre, int64_t first = 0, int k = 50) {
        using namespace spaghetti;
        if (!lexicon) throw std::runtime_error("WordList: no lexicon (SetLexicon)");
        const uint32_t p_ptr[2] = {0u, (uint32_t)pre.size()};
        std::vector<uint32_t> ids((size_t)std::max(k, 1));
        int32_t n = 0;
        check(ss_lexicon_prefix(lexicon, 1, p_ptr, reinterpret_cast<const uint8_t*>(pre.data()), first, k, ids.data(), &n, nullptr), "ss_lexicon_prefix");
        std::vector<std::string> out;
        for (int32_t i = 0; i < n; i++) out.push_back(lex_words[ids[i]]);
        return out;
    }
    // Per token of `query` that the index does not know (SS_UNKNOWN_TERM in Retrieve), the m known words within max_dist byte edits
    // whose frequency is at least 1; nothing for known tokens.  The query is tokenised as ExplainResults does it.
    std::vector<WordSuggestion> SuggestWords(const std::string& query, int max_dist = 2, int m = 5) {
        using namespace spaghetti;
        if (!lexicon) throw std::runtime_error("SuggestWords: no lexicon (SetLexicon)");
        std::vector<WordSuggestion> out;
        std::vector<uint32_t> w_ptr{0};
        std::string bytes;
        for (auto& w : query_words(query)) {
            if (terms.id.find(md5::hex(w)) != terms.id.end()) continue;
            bool seen = false;
            for (auto& o : out) seen = seen || o.Token == w;
            if (seen) continue;
            out.push_back(WordSuggestion{w, {}, {}, {}});
            bytes += w;
            w_ptr.push_back((uint32_t)bytes.size());
        }
        if (out.empty()) return out;
        const size_t nq = out.size(), mm = (size_t)std::max(m, 1);
        std::vector<uint32_t> ids(nq * mm);
        std::vector<int32_t> dist(nq * mm), n(nq);
        check(ss_lexicon_suggest(lexicon, (int32_t)nq, w_ptr.data(), reinterpret_cast<const uint8_t*>(bytes.data()), max_dist, 1u, m, ids.data(),
                                 dist.data(), n.data()), "ss_lexicon_suggest");
        for (size_t q = 0; q < nq; q++)
            for (int32_t r = 0; r < n[q]; r++) {
                const uint32_t t = ids[q * mm + r];
                out[q].Words.push_back(lex_words[t]);
                out[q].Distances.push_back(dist[q * mm + r]);
                out[q].Freqs.push_back(lex_freq[t]);
            }
        return out;
    }
    // "Results while you type", the word half: the m most frequent words of the vocabulary that start with `pre` and whose frequency is
    // at least min_freq, best first (ss_lexicon_complete).  `pre` is taken byte for byte: the caller lower-cases it as it sees fit.
    std::vector<WordCompletion> Complete(const std::string& pre, int m = 10, uint32_t min_freq = 1) {
        using namespace spaghetti;
        if (!lexicon) throw std::runtime_error("Complete: no lexicon (SetLexicon)");
        const uint32_t p_ptr[2] = {0u, (uint32_t)pre.size()};
        std::vector<uint32_t> ids((size_t)std::max(m, 1)), freq((size_t)std::max(m, 1));
        int32_t n = 0;
        check(ss_lexicon_complete(lexicon, 1, p_ptr, reinterpret_cast<const uint8_t*>(pre.data()), min_freq, m, ids.data(), freq.data(), &n, nullptr),
              "ss_lexicon_complete");
        std::vector<WordCompletion> out;
        for (int32_t i = 0; i < n; i++) out.push_back(WordCompletion{lex_words[ids[i]], freq[i]});
        return out;
    }
    // ... and the query half (default 0: off, every string is read exactly as before).  With 1 <= expansions <= 32, every entry point
    // that tokenises query strings the way RetrieveBatch does reads a token written `word*` outside quoted phrases as a prefix term:
    // the token leaves the string the tokeniser sees (as "-word" tokens do under SetQueryOperators), its bytes are lower-cased, NOT
    // stemmed, and the `expansions` most frequent words that start with them (frequency at least 1) join the query as plain OR terms
    // behind its words; a prefix without a completion counts as one unknown word.  The token adds 1 to the query's length, whatever
    // it expands to, and a query is cut at SS_MAX_QUERY_TERMS terms.  The lexicon holds the words as the indexer stemmed them, so
    // "runn*" does not find "run": a prefix is matched against stems.  Under SetQueryOperators "+word*" and "-word*" stay operator
    // tokens.  Entry points that refuse query operators refuse this setting too; ExplainResults, BestPassages and SuggestWords read
    // the string without it.  Needs SetLexicon (again after load()): a prefix token without a lexicon throws.
    void SetPrefixQueries(int expansions) {
        if (expansions < 0 || expansions > 32) throw std::runtime_error("SetPrefixQueries: expansions must be 0 (off) or 1 .. 32");
        prefix_expansions = expansions;
    }
    // Per row of `results` — the Rank_combined rows Retrieve / RetrieveBatch returned for `query` — the best body window of `width`
    // word positions (ss_best_passages).  The query is tokenised as ExplainResults does it.  A row whose DocHash the index does not
    // hold has no passage.  Changes nothing unless called.
    std::vector<ResultPassage> BestPassages(const std::string& query, const std::vector<Rank_combined>& results, int width = 20) {
        using namespace spaghetti;
        const std::vector<std::string> hashed = query_word_hashes(query);
        std::vector<ResultPassage> out(results.size());
        if (results.empty()) return out;
        const size_t k = results.size(), T = hashed.size();
        if (T == 0) return out;
        if (k > (size_t)SS_MAX_TOPK || T > (size_t)SS_MAX_QUERY_TERMS) throw std::runtime_error("BestPassages: too many rows or query words");
        std::vector<uint32_t> q_ptr{0, (uint32_t)T}, q_terms;
        for (auto& h : hashed) {
            auto it = terms.id.find(h);
            q_terms.push_back(it == terms.id.end() ? SS_UNKNOWN_TERM : it->second);
        }
        std::vector<ss_hit> hits(k);
        for (size_t j = 0; j < k; j++) {
            auto it = docs.id.find(results[j].DocHash);
            hits[j] = ss_hit{};
            hits[j].doc = it == docs.id.end() ? 0xFFFFFFFFu : it->second;      // no such doc: no postings
        }
        const int32_t n_hits = (int32_t)k;
        std::vector<ss_passage> m(k);
        check(ss_best_passages(scorer, 1, q_ptr.data(), q_terms.data(), (int32_t)k, hits.data(), &n_hits, (int32_t)width, m.data()), "ss_best_passages");
        for (size_t j = 0; j < k; j++) {
            if (!m[j].n_occ) continue;
            out[j].HasPassage = true;
            out[j].Start = (double)m[j].start;
            out[j].Last = (double)m[j].last;
            out[j].Distinct = m[j].n_distinct;
            out[j].Occurrences = m[j].n_occ;
            for (size_t i = 0; i < T; i++)
                if (((m[j].token_mask >> i) & 1u) && std::find(out[j].Words.begin(), out[j].Words.end(), hashed[i]) == out[j].Words.end())
                    out[j].Words.push_back(hashed[i]);
        }
        return out;
    }
    // one ss_proximity entry as the host's struct; names: the query's tokens as word hashes, in token order
    static ResultProximity to_proximity(const ss_proximity& e, const std::vector<std::string>& names) {
        ResultProximity r;
        if (!e.n_present) return r;
        r.HasSpan = true;
        r.Start = (double)e.start;
        r.End = (double)e.end;
        r.Present = e.n_present;
        r.Occurrences = e.n_occ;
        for (size_t i = 0; i < names.size() && i < 64; i++)
            if (((e.token_mask >> i) & 1u) && std::find(r.Words.begin(), r.Words.end(), names[i]) == r.Words.end()) r.Words.push_back(names[i]);
        return r;
    }
    // Per row of `results` — the Rank_combined rows Retrieve / RetrieveBatch returned for `query` — the smallest body span that holds
    // every query word the page has (ss_hit_proximity).  The query is tokenised as ExplainResults does it.  A row whose DocHash the
    // index does not hold has no span.  Changes nothing unless called.
    std::vector<ResultProximity> HitProximity(const std::string& query, const std::vector<Rank_combined>& results) {
        using namespace spaghetti;
        const std::vector<std::string> hashed = query_word_hashes(query);
        std::vector<ResultProximity> out(results.size());
        if (results.empty()) return out;
        const size_t k = results.size(), T = hashed.size();
        if (T == 0) return out;
        if (k > (size_t)SS_MAX_TOPK || T > (size_t)SS_MAX_QUERY_TERMS) throw std::runtime_error("HitProximity: too many rows or query words");
        std::vector<uint32_t> q_ptr{0, (uint32_t)T}, q_terms;
        for (auto& h : hashed) {
            auto it = terms.id.find(h);
            q_terms.push_back(it == terms.id.end() ? SS_UNKNOWN_TERM : it->second);
        }
        std::vector<ss_hit> hits(k);
        for (size_t j = 0; j < k; j++) {
            auto it = docs.id.find(results[j].DocHash);
            hits[j] = ss_hit{};
            hits[j].doc = it == docs.id.end() ? 0xFFFFFFFFu : it->second;      // no such doc: no postings
        }
        const int32_t n_hits = (int32_t)k;
        std::vector<ss_proximity> m(k);
        check(ss_hit_proximity(scorer, 1, q_ptr.data(), q_terms.data(), (int32_t)k, hits.data(), &n_hits, m.data()), "ss_hit_proximity");
        for (size_t j = 0; j < k; j++) out[j] = to_proximity(m[j], hashed);
        return out;
    }
    // dense term ids -> word hashes (DocTopTerms, RelatedTerms)
    std::vector<std::string> term_hashes(const uint32_t* ids, int32_t n) const {
        std::vector<std::string> out;
        for (int32_t i = 0; i < n; i++) out.push_back(terms.name[ids[i]]);
        return out;
    }

    // Replace the named allow-lists: name -> doc hashes (hashes the index does not hold are ignored).
    void SetDocMasks(const std::map<std::string, std::vector<std::string>>& sets) {
        mask_sets = sets;
        register_masks();
    }
    // mask_sets -> the scorer's doc masks (ss_scorer_set_doc_masks), in name order
    void register_masks() {
        using namespace spaghetti;
        mask_index.clear();
        if (!scorer || !title) return;
        uint64_t n = 0, nt = 0, np = 0;
        check(ss_index_get_info(title, &n, &nt, &np), "ss_index_get_info");
        const size_t W = (size_t)((n + 31) / 32);
        std::vector<uint32_t> words(mask_sets.size() * W, 0u);
        int32_t m = 0;
        for (auto& kv : mask_sets) {
            uint32_t* row = words.data() + (size_t)m * W;
            for (auto& d : kv.second) {
                auto it = docs.id.find(d);
                if (it != docs.id.end() && it->second < n) row[it->second >> 5] |= 1u << (it->second & 31);
            }
            mask_index[kv.first] = m++;
        }
        check(ss_scorer_set_doc_masks(scorer, m, m ? words.data() : nullptr), "ss_scorer_set_doc_masks");
    }

    // Site keys for collapsed pages: doc hash -> key string (the caller's: a host name, a registrable domain; this mirror holds no
    // URLs — the reference's forw[1] does).  Equal strings are one site; docs not named are never collapsed (SS_NO_GROUP); hashes
    // the index does not hold are ignored.
    void SetDocGroups(const std::map<std::string, std::string>& keys) {
        doc_group_keys = keys;
        has_doc_groups = true;
        register_groups();
    }
    // doc_group_keys -> the scorer's group table (ss_scorer_set_doc_groups): a key's number is its rank among the distinct keys
    void register_groups() {
        using namespace spaghetti;
        if (!has_doc_groups || !scorer || !title) return;
        uint64_t n = 0, nt = 0, np = 0;
        check(ss_index_get_info(title, &n, &nt, &np), "ss_index_get_info");
        std::map<std::string, uint32_t> number;
        for (auto& kv : doc_group_keys) number.emplace(kv.second, 0u);
        uint32_t next = 0;
        doc_group_names.clear();
        for (auto& kv : number) {
            kv.second = next++;
            doc_group_names.push_back(kv.first);
        }
        std::vector<uint32_t> group((size_t)n, SS_NO_GROUP);
        for (auto& kv : doc_group_keys) {
            auto it = docs.id.find(kv.first);
            if (it != docs.id.end() && it->second < n) group[it->second] = number[kv.second];
        }
        check(ss_scorer_set_doc_groups(scorer, group.data()), "ss_scorer_set_doc_groups");
    }

    // Doc fields for range filters and sorting: doc hash -> {Mod_date as unix seconds, Page_size in bytes}, field 0 and field 1 of the
    // scorer's table.  A doc the map does not name has SS_NO_FIELD_VALUE in both fields (no sensible range matches it); hashes the
    // index does not hold are ignored.
    void SetDocFields(const std::map<std::string, std::pair<int64_t, int64_t>>& fields) {
        doc_field_values = fields;
        has_doc_fields = true;
        register_fields();
    }
    void register_fields() {
        using namespace spaghetti;
        if (!has_doc_fields || !scorer || !title) return;
        uint64_t n = 0, nt = 0, np = 0;
        check(ss_index_get_info(title, &n, &nt, &np), "ss_index_get_info");
        std::vector<int64_t> values(2 * (size_t)n, SS_NO_FIELD_VALUE);
        for (auto& kv : doc_field_values) {
            auto it = docs.id.find(kv.first);
            if (it == docs.id.end() || it->second >= n) continue;
            values[it->second] = kv.second.first;
            values[(size_t)n + it->second] = kv.second.second;
        }
        check(ss_scorer_set_doc_fields(scorer, 2, values.data()), "ss_scorer_set_doc_fields");
    }

    // Doc vectors for VectorSearch / RerankByVector: doc hash -> int8 embedding, all of one length (a multiple of 64 up to
    // SS_MAX_VEC_DIM).  A doc the map does not name has the zero vector (score 0 under every query); hashes the index does not hold
    // are ignored.  An empty map clears the table.
    void SetDocVectors(const std::map<std::string, std::vector<int8_t>>& vectors) {
        int dim = 0;
        for (auto& kv : vectors) {
            if (dim == 0) dim = (int)kv.second.size();
            if ((int)kv.second.size() != dim) throw std::runtime_error("SetDocVectors: vectors of different lengths");
        }
        if (!vectors.empty() && (dim < 64 || dim > SS_MAX_VEC_DIM || dim % 64))
            throw std::runtime_error("SetDocVectors: the length must be a multiple of 64 in [64, SS_MAX_VEC_DIM]");
        doc_vectors = vectors;
        doc_vector_dim = dim;
        list_centroids.clear();                                                 // (the lists describe the old table)
        n_vector_lists = 0;
        register_vectors();
    }
    void register_vectors() {
        using namespace spaghetti;
        if (!scorer || !title) return;
        if (doc_vector_dim == 0) { check(ss_scorer_set_doc_vectors(scorer, 0, nullptr), "ss_scorer_set_doc_vectors"); return; }
        uint64_t n = 0, nt = 0, np = 0;
        check(ss_index_get_info(title, &n, &nt, &np), "ss_index_get_info");
        std::vector<int8_t> table((size_t)n * doc_vector_dim, 0);
        for (auto& kv : doc_vectors) {
            auto it = docs.id.find(kv.first);
            if (it == docs.id.end() || it->second >= n) continue;
            std::copy(kv.second.begin(), kv.second.end(), table.begin() + (size_t)it->second * doc_vector_dim);
        }
        check(ss_scorer_set_doc_vectors(scorer, doc_vector_dim, table.data()), "ss_scorer_set_doc_vectors");
        register_vector_lists();
    }
    // Doc tokens for RerankByMaxSim: doc hash -> its token vectors, all of one length (a multiple of 64 up to SS_MAX_VEC_DIM).  A doc
    // the map does not name, or names with no vector, has no token and so no score; hashes the index does not hold are ignored.  An
    // empty map clears the table.  Independent of SetDocVectors.
    void SetDocTokens(const std::map<std::string, std::vector<std::vector<int8_t>>>& tokens) {
        int dim = 0;
        for (auto& kv : tokens)
            for (auto& v : kv.second) {
                if (dim == 0) dim = (int)v.size();
                if ((int)v.size() != dim) throw std::runtime_error("SetDocTokens: token vectors of different lengths");
            }
        if (dim != 0 && (dim < 64 || dim > SS_MAX_VEC_DIM || dim % 64))
            throw std::runtime_error("SetDocTokens: the length must be a multiple of 64 in [64, SS_MAX_VEC_DIM]");
        doc_tokens = tokens;
        doc_token_dim = dim;
        register_tokens();
    }
    void register_tokens() {
        using namespace spaghetti;
        if (!scorer || !title) return;
        if (doc_token_dim == 0) { check(ss_scorer_set_doc_tokens(scorer, 0, nullptr, nullptr), "ss_scorer_set_doc_tokens"); return; }
        uint64_t n = 0, nt = 0, np = 0;
        check(ss_index_get_info(title, &n, &nt, &np), "ss_index_get_info");
        std::vector<const std::vector<std::vector<int8_t>>*> of_doc((size_t)n, nullptr);
        for (auto& kv : doc_tokens) {
            auto it = docs.id.find(kv.first);
            if (it == docs.id.end() || it->second >= n) continue;
            of_doc[it->second] = &kv.second;
        }
        std::vector<uint64_t> tok_ptr((size_t)n + 1, 0);
        for (size_t d = 0; d < (size_t)n; d++) tok_ptr[d + 1] = tok_ptr[d] + (of_doc[d] ? of_doc[d]->size() : 0);
        std::vector<int8_t> table((size_t)tok_ptr[n] * doc_token_dim + 1, 0);    // (+ 1: never an empty array, which would clear)
        for (size_t d = 0; d < (size_t)n; d++) {
            if (!of_doc[d]) continue;
            size_t row = (size_t)tok_ptr[d];
            for (auto& v : *of_doc[d]) std::copy(v.begin(), v.end(), table.begin() + (row++) * doc_token_dim);
        }
        check(ss_scorer_set_doc_tokens(scorer, doc_token_dim, tok_ptr.data(), table.data()), "ss_scorer_set_doc_tokens");
    }
    // Vector lists for VectorSearchProbed: n_lists centroids of the vectors' length.  Every doc goes to the list of the centroid with
    // the largest integer dot product (ties to the lower list), assigned on the device; no centroids clears the lists.
    void SetVectorLists(int n_lists, const std::vector<std::vector<int8_t>>& centroids) {
        using namespace spaghetti;
        if (n_lists < 0 || (size_t)n_lists != centroids.size()) throw std::runtime_error("SetVectorLists: n_lists centroids are needed");
        if (!centroids.empty() && doc_vector_dim == 0) throw std::runtime_error("SetVectorLists: no doc vectors (SetDocVectors)");
        if (centroids.size() > (size_t)SS_MAX_VEC_LISTS) throw std::runtime_error("SetVectorLists: more than SS_MAX_VEC_LISTS lists");
        std::vector<int8_t> flat;
        for (auto& c : centroids) {
            if ((int)c.size() != doc_vector_dim) throw std::runtime_error("SetVectorLists: a centroid of the wrong length");
            flat.insert(flat.end(), c.begin(), c.end());
        }
        list_centroids = std::move(flat);
        n_vector_lists = (int)centroids.size();
        if (n_vector_lists == 0 && scorer && doc_vector_dim) check(ss_scorer_set_vector_lists(scorer, 0, nullptr, nullptr), "ss_scorer_set_vector_lists");
        register_vector_lists();
    }
    void register_vector_lists() {
        using namespace spaghetti;
        if (!scorer || !title || n_vector_lists == 0 || doc_vector_dim == 0) return;
        uint64_t n = 0, nt = 0, np = 0;
        check(ss_index_get_info(title, &n, &nt, &np), "ss_index_get_info");
        std::vector<uint32_t> list_of_doc((size_t)n);
        check(ss_vector_assign_lists(scorer, n_vector_lists, list_centroids.data(), list_of_doc.data(), nullptr), "ss_vector_assign_lists");
        check(ss_scorer_set_vector_lists(scorer, n_vector_lists, list_centroids.data(), list_of_doc.data()), "ss_scorer_set_vector_lists");
    }
    std::vector<int8_t> flatten_query_vectors(const char* who, const std::vector<std::vector<int8_t>>& queryVectors) const {
        if (doc_vector_dim == 0) throw std::runtime_error(std::string(who) + ": no doc vectors (SetDocVectors)");
        std::vector<int8_t> flat;
        for (auto& v : queryVectors) {
            if ((int)v.size() != doc_vector_dim) throw std::runtime_error(std::string(who) + ": a query vector of the wrong length");
            flat.insert(flat.end(), v.begin(), v.end());
        }
        return flat;
    }
    // Exact nearest neighbours: per query vector the k docs of the largest integer dot product, ties by dense doc id, among the docs of
    // the set masks[q] names (SetDocMasks; "" or an empty list: the whole index).
    std::vector<std::vector<VectorHit>> VectorSearch(const std::vector<std::vector<int8_t>>& queryVectors, int k = 50,
                                                     const std::vector<std::string>& masks = {}) {
        using namespace spaghetti;
        const std::vector<int8_t> flat = flatten_query_vectors("VectorSearch", queryVectors);
        const size_t nq = queryVectors.size();
        if (!masks.empty() && masks.size() != nq) throw std::runtime_error("VectorSearch: one mask name per query");
        std::vector<int32_t> mask_id(nq, -1);
        for (size_t q = 0; q < masks.size(); q++) {
            if (masks[q].empty()) continue;
            auto it = mask_index.find(masks[q]);
            if (it == mask_index.end()) throw std::runtime_error("VectorSearch: no doc mask named '" + masks[q] + "' (SetDocMasks)");
            mask_id[q] = it->second;
        }
        std::vector<ss_vec_hit> hits(nq * (size_t)std::max(k, 1));
        std::vector<int32_t> n_hits(nq);
        check(ss_vector_topk(scorer, (int32_t)nq, flat.data(), mask_id.data(), k, hits.data(), n_hits.data()), "ss_vector_topk");
        std::vector<std::vector<VectorHit>> out(nq);
        for (size_t q = 0; q < nq; q++)
            for (int i = 0; i < n_hits[q]; i++) {
                const ss_vec_hit& h = hits[q * (size_t)k + i];
                out[q].push_back(VectorHit{docs.name[h.doc], h.score});
            }
        return out;
    }
    // VectorSearch over the docs of the n_probe lists (SetVectorLists) whose centroids score highest under the query: exact within
    // them, and VectorSearch's rows when every list is probed.
    std::vector<std::vector<VectorHit>> VectorSearchProbed(const std::vector<std::vector<int8_t>>& queryVectors, int k = 50, int n_probe = 8,
                                                           const std::vector<std::string>& masks = {}) {
        using namespace spaghetti;
        const std::vector<int8_t> flat = flatten_query_vectors("VectorSearchProbed", queryVectors);
        if (n_vector_lists == 0) throw std::runtime_error("VectorSearchProbed: no vector lists (SetVectorLists)");
        const size_t nq = queryVectors.size();
        if (!masks.empty() && masks.size() != nq) throw std::runtime_error("VectorSearchProbed: one mask name per query");
        std::vector<int32_t> mask_id(nq, -1);
        for (size_t q = 0; q < masks.size(); q++) {
            if (masks[q].empty()) continue;
            auto it = mask_index.find(masks[q]);
            if (it == mask_index.end()) throw std::runtime_error("VectorSearchProbed: no doc mask named '" + masks[q] + "' (SetDocMasks)");
            mask_id[q] = it->second;
        }
        std::vector<ss_vec_hit> hits(nq * (size_t)std::max(k, 1));
        std::vector<int32_t> n_hits(nq);
        check(ss_vector_topk_probed(scorer, (int32_t)nq, flat.data(), mask_id.data(), k, n_probe, hits.data(), n_hits.data(), nullptr),
              "ss_vector_topk_probed");
        std::vector<std::vector<VectorHit>> out(nq);
        for (size_t q = 0; q < nq; q++)
            for (int i = 0; i < n_hits[q]; i++) {
                const ss_vec_hit& h = hits[q * (size_t)k + i];
                out[q].push_back(VectorHit{docs.name[h.doc], h.score});
            }
        return out;
    }
    // A window of result rows per query (RetrieveBatch's, or any other call's) re-ordered by vector score, descending and stable;
    // page [first, first + k).  Rows whose doc hash the index does not hold come last.
    std::vector<VectorRerankedPage> RerankByVector(const std::vector<std::vector<int8_t>>& queryVectors,
                                                   const std::vector<std::vector<Rank_combined>>& rows, int first = 0, int k = 50) {
        using namespace spaghetti;
        const std::vector<int8_t> flat = flatten_query_vectors("RerankByVector", queryVectors);
        const size_t nq = queryVectors.size(), kk = (size_t)std::max(k, 1);
        if (rows.size() != nq) throw std::runtime_error("RerankByVector: one window per query vector");
        size_t k_in = 1;
        for (auto& r : rows) k_in = std::max(k_in, r.size());
        std::vector<ss_hit> win(nq * k_in), page(nq * kk);
        std::vector<int32_t> n_rows(nq), n_page(nq), scores(nq * kk);
        for (size_t q = 0; q < nq; q++) {
            n_rows[q] = (int32_t)rows[q].size();
            for (size_t j = 0; j < rows[q].size(); j++) {
                const Rank_combined& r = rows[q][j];
                auto it = docs.id.find(r.DocHash);
                ss_hit h{};
                h.doc = it == docs.id.end() ? 0xFFFFFFFFu : it->second;
                h._pad = (uint32_t)j;                                     // the window position: how the page finds its row again
                h.title = r.TitleRank; h.body = r.BodyRank; h.pagerank = r.PageRank; h.final = r.FinalRank;
                win[q * k_in + j] = h;
            }
        }
        check(ss_rerank_hits_by_vector(scorer, (int32_t)nq, flat.data(), (int32_t)k_in, win.data(), n_rows.data(), first, k, page.data(),
                                       n_page.data(), scores.data()), "ss_rerank_hits_by_vector");
        std::vector<VectorRerankedPage> out(nq);
        for (size_t q = 0; q < nq; q++)
            for (int i = 0; i < n_page[q]; i++) {
                out[q].Results.push_back(rows[q][page[q * kk + i]._pad]);
                out[q].Scores.push_back(scores[q * kk + i]);
            }
        return out;
    }

    // A window of result rows per query re-ordered by late-interaction score (ss_rerank_hits_by_maxsim): the sum, over the query's
    // token vectors, of the best dot product any of the doc's token vectors reaches; descending and stable; page [first, first + k).
    // queryTokens[q]: at most SS_MAX_QUERY_TOKENS vectors of the tokens' length.  Rows whose doc has no token, or whose doc hash the
    // index does not hold, come last with SS_NO_VEC_SCORE.
    std::vector<VectorRerankedPage> RerankByMaxSim(const std::vector<std::vector<std::vector<int8_t>>>& queryTokens,
                                                   const std::vector<std::vector<Rank_combined>>& rows, int first = 0, int k = 50) {
        using namespace spaghetti;
        if (doc_token_dim == 0) throw std::runtime_error("RerankByMaxSim: no doc tokens (SetDocTokens)");
        const size_t nq = queryTokens.size(), kk = (size_t)std::max(k, 1);
        if (rows.size() != nq) throw std::runtime_error("RerankByMaxSim: one window per query");
        std::vector<uint32_t> qt_ptr(nq + 1, 0);
        std::vector<int8_t> flat;
        for (size_t q = 0; q < nq; q++) {
            for (auto& v : queryTokens[q]) {
                if ((int)v.size() != doc_token_dim) throw std::runtime_error("RerankByMaxSim: a query token vector of the wrong length");
                flat.insert(flat.end(), v.begin(), v.end());
            }
            qt_ptr[q + 1] = qt_ptr[q] + (uint32_t)queryTokens[q].size();
        }
        size_t k_in = 1;
        for (auto& r : rows) k_in = std::max(k_in, r.size());
        std::vector<ss_hit> win(nq * k_in), page(nq * kk);
        std::vector<int32_t> n_rows(nq), n_page(nq), scores(nq * kk);
        for (size_t q = 0; q < nq; q++) {
            n_rows[q] = (int32_t)rows[q].size();
            for (size_t j = 0; j < rows[q].size(); j++) {
                const Rank_combined& r = rows[q][j];
                auto it = docs.id.find(r.DocHash);
                ss_hit h{};
                h.doc = it == docs.id.end() ? 0xFFFFFFFFu : it->second;
                h._pad = (uint32_t)j;                                     // the window position: how the page finds its row again
                h.title = r.TitleRank; h.body = r.BodyRank; h.pagerank = r.PageRank; h.final = r.FinalRank;
                win[q * k_in + j] = h;
            }
        }
        check(ss_rerank_hits_by_maxsim(scorer, (int32_t)nq, qt_ptr.data(), flat.data(), (int32_t)k_in, win.data(), n_rows.data(), first, k,
                                       page.data(), n_page.data(), scores.data()), "ss_rerank_hits_by_maxsim");
        std::vector<VectorRerankedPage> out(nq);
        for (size_t q = 0; q < nq; q++)
            for (int i = 0; i < n_page[q]; i++) {
                out[q].Results.push_back(rows[q][page[q * kk + i]._pad]);
                out[q].Scores.push_back(scores[q * kk + i]);
            }
        return out;
    }

    // The k docs with the highest late-interaction score under each query's token vectors, over every doc that has a token
    // (ss_maxsim_topk: exact, score descending, then doc id ascending), by doc name.  queryTokens[q] as in RerankByMaxSim (an empty
    // query scores every doc 0); masks: empty, or one name per query ("" = every doc) of a mask of SetDocMasks.
    std::vector<std::vector<VectorHit>> MaxSimSearch(const std::vector<std::vector<std::vector<int8_t>>>& queryTokens, int k = 50,
                                                     const std::vector<std::string>& masks = {}) {
        using namespace spaghetti;
        if (doc_token_dim == 0) throw std::runtime_error("MaxSimSearch: no doc tokens (SetDocTokens)");
        const size_t nq = queryTokens.size();
        if (!masks.empty() && masks.size() != nq) throw std::runtime_error("MaxSimSearch: one mask name per query");
        std::vector<uint32_t> qt_ptr(nq + 1, 0);
        std::vector<int8_t> flat;
        for (size_t q = 0; q < nq; q++) {
            for (auto& v : queryTokens[q]) {
                if ((int)v.size() != doc_token_dim) throw std::runtime_error("MaxSimSearch: a query token vector of the wrong length");
                flat.insert(flat.end(), v.begin(), v.end());
            }
            qt_ptr[q + 1] = qt_ptr[q] + (uint32_t)queryTokens[q].size();
        }
        std::vector<int32_t> mask_id(nq, -1);
        for (size_t q = 0; q < masks.size(); q++) {
            if (masks[q].empty()) continue;
            auto it = mask_index.find(masks[q]);
            if (it == mask_index.end()) throw std::runtime_error("MaxSimSearch: no doc mask named '" + masks[q] + "' (SetDocMasks)");
            mask_id[q] = it->second;
        }
        std::vector<ss_vec_hit> hits(nq * (size_t)std::max(k, 1));
        std::vector<int32_t> n_hits(nq);
        check(ss_maxsim_topk(scorer, (int32_t)nq, qt_ptr.data(), flat.empty() ? nullptr : flat.data(), mask_id.data(), k, hits.data(),
                             n_hits.data()), "ss_maxsim_topk");
        std::vector<std::vector<VectorHit>> out(nq);
        for (size_t q = 0; q < nq; q++)
            for (int i = 0; i < n_hits[q]; i++) {
                const ss_vec_hit& h = hits[q * (size_t)k + i];
                out[q].push_back(VectorHit{docs.name[h.doc], h.score});
            }
        return out;
    }

    // A window of result rows per query re-ranked greedily (ss_diversify_hits): every next row is the one with the largest w_rel *
    // relevance - w_div * (largest similarity of its doc vector to a row already chosen), of equal values the earlier row; page
    // [first, first + k).  Relevance is the row's score under the query's vector, or, with queryVectors EMPTY, minus its position in the
    // window: that diversifies a lexical window which keeps its own order.  The weights are integers in [0, SS_DIV_WEIGHT_MAX].  Rows
    // whose doc hash the index does not hold come last.
    std::vector<DiversifiedPage> DiversifyByVector(const std::vector<std::vector<int8_t>>& queryVectors,
                                                   const std::vector<std::vector<Rank_combined>>& rows, int w_rel, int w_div, int first = 0,
                                                   int k = 50) {
        using namespace spaghetti;
        const bool by_rank = queryVectors.empty();
        const std::vector<int8_t> flat = flatten_query_vectors("DiversifyByVector", queryVectors);
        const size_t nq = rows.size(), kk = (size_t)std::max(k, 1);
        if (!by_rank && queryVectors.size() != nq) throw std::runtime_error("DiversifyByVector: one window per query vector");
        size_t k_in = 1;
        for (auto& r : rows) k_in = std::max(k_in, r.size());
        std::vector<ss_hit> win(nq * k_in), page(nq * kk);
        std::vector<int32_t> n_rows(nq), n_page(nq);
        std::vector<ss_div_info> info(nq * kk);
        for (size_t q = 0; q < nq; q++) {
            n_rows[q] = (int32_t)rows[q].size();
            for (size_t j = 0; j < rows[q].size(); j++) {
                const Rank_combined& r = rows[q][j];
                auto it = docs.id.find(r.DocHash);
                ss_hit h{};
                h.doc = it == docs.id.end() ? 0xFFFFFFFFu : it->second;
                h._pad = (uint32_t)j;                                     // the window position: how the page finds its row again
                h.title = r.TitleRank; h.body = r.BodyRank; h.pagerank = r.PageRank; h.final = r.FinalRank;
                win[q * k_in + j] = h;
            }
        }
        check(ss_diversify_hits(scorer, (int32_t)nq, by_rank ? nullptr : flat.data(), (int32_t)k_in, win.data(), n_rows.data(), w_rel, w_div,
                                first, k, page.data(), n_page.data(), info.data()), "ss_diversify_hits");
        std::vector<DiversifiedPage> out(nq);
        for (size_t q = 0; q < nq; q++)
            for (int i = 0; i < n_page[q]; i++) {
                out[q].Results.push_back(rows[q][page[q * kk + i]._pad]);
                out[q].Rel.push_back(info[q * kk + i].rel);
                out[q].Sim.push_back(info[q * kk + i].sim);
            }
        return out;
    }

    // The row that a query's ranking holds for each of the given docs, whether or not the doc would reach any top-k (ss_score_docs): the
    // FinalRank of the output of VectorSearch, SimilarPages or TopLinks.  A doc hash the index does not hold gives a row of zeros
    // under its hash.  Quoted phrases and query operators are not read here: they decide which docs rank, not a doc's row.
    std::vector<Rank_combined> ScoreDocs(const std::string& query, const std::vector<std::string>& docHashes,
                                         const std::map<std::string, double>* topicProbs = nullptr, bool live_topic_probs = false) {
        using namespace spaghetti;
        std::vector<std::map<std::string, double>> tp;
        if (topicProbs) tp.push_back(*topicProbs);
        const Tokenised t = tokenise({query}, topicProbs ? &tp : nullptr, live_topic_probs);
        if (!t.p_terms.empty()) throw std::runtime_error("ScoreDocs: quoted phrases are not read here");
        std::vector<Rank_combined> out(docHashes.size());
        for (size_t lo = 0; lo < docHashes.size(); lo += SS_MAX_TOPK) {
            const size_t n = std::min<size_t>(SS_MAX_TOPK, docHashes.size() - lo);
            std::vector<uint32_t> ids(n);
            for (size_t j = 0; j < n; j++) {
                auto it = docs.id.find(docHashes[lo + j]);
                ids[j] = it == docs.id.end() ? 0xFFFFFFFFu : it->second;
            }
            std::vector<ss_hit> rows(n);
            const int32_t n_in = (int32_t)n;
            check(ss_score_docs(scorer, 1, t.q_ptr.data(), t.q_terms.data(), t.q_len.data(), t.probs.empty() ? nullptr : t.probs.data(), (int32_t)n,
                                ids.data(), &n_in, rows.data()), "ss_score_docs");
            for (size_t j = 0; j < n; j++) {
                Rank_combined& r = out[lo + j];
                r.DocHash = docHashes[lo + j];
                r.PageRank = rows[j].pagerank; r.FinalRank = rows[j].final; r.TitleRank = rows[j].title; r.BodyRank = rows[j].body;
            }
        }
        return out;
    }
    // Lexical and vector search fused (ss_hybrid_topk): per query the first k_window rows of its lexical ranking and the k_window
    // nearest docs of its vector, both among the docs of the set masks[q] names (SetDocMasks; "" or an empty list: the whole index),
    // merged into one ranking by `params`; page [first, first + k).  A doc only one window holds is completed on the device, so every
    // row carries its FinalRank and its vector score.  Quoted phrases and query operators are not read here.
    std::vector<HybridPage> HybridSearch(const std::vector<std::string>& queries, const std::vector<std::vector<int8_t>>& queryVectors,
                                         int k_window, const HybridParams& params = HybridParams(), int first = 0, int k = 50,
                                         const std::vector<std::string>& masks = {},
                                         const std::vector<std::map<std::string, double>>* topicProbs = nullptr, bool live_topic_probs = false) {
        using namespace spaghetti;
        const std::vector<int8_t> flat = flatten_query_vectors("HybridSearch", queryVectors);
        const size_t nq = queries.size(), kk = (size_t)std::max(k, 1);
        if (queryVectors.size() != nq) throw std::runtime_error("HybridSearch: one query vector per query");
        if (!masks.empty() && masks.size() != nq) throw std::runtime_error("HybridSearch: one mask name per query");
        if (query_operators) throw std::runtime_error("HybridSearch: query operators are not read here (SetQueryOperators(false))");
        if (prefix_expansions) throw std::runtime_error("HybridSearch: prefix queries are not read here (SetPrefixQueries(0))");
        std::vector<int32_t> mask_id(nq, -1);
        for (size_t q = 0; q < masks.size(); q++) {
            if (masks[q].empty()) continue;
            auto it = mask_index.find(masks[q]);
            if (it == mask_index.end()) throw std::runtime_error("HybridSearch: no doc mask named '" + masks[q] + "' (SetDocMasks)");
            mask_id[q] = it->second;
        }
        const Tokenised t = tokenise(queries, topicProbs, live_topic_probs);
        if (!t.p_terms.empty()) throw std::runtime_error("HybridSearch: quoted phrases are not read here");
        const ss_fuse_params fp{params.weighted ? SS_FUSE_WEIGHTED : SS_FUSE_RRF, params.rrf_c, params.w_lex, params.w_vec};
        std::vector<ss_hit> page(nq * kk);
        std::vector<ss_fused> fused(nq * kk);
        std::vector<int32_t> n_page(nq), n_union(nq);
        check(ss_hybrid_topk(scorer, t.nq, t.q_ptr.data(), t.q_terms.data(), t.q_len.data(), t.probs.empty() ? nullptr : t.probs.data(),
                             flat.data(), mask_id.data(), k_window, &fp, first, k, page.data(), n_page.data(), fused.data(), n_union.data()),
              "ss_hybrid_topk");
        const std::vector<std::vector<Rank_combined>> ranks = to_ranks(t.nq, k, page, n_page);
        std::vector<HybridPage> out(nq);
        for (size_t q = 0; q < nq; q++) {
            out[q].Results = ranks[q];
            out[q].Union = n_union[q];
            for (int i = 0; i < n_page[q]; i++) {
                const ss_fused& f = fused[q * kk + i];
                out[q].Scores.push_back(f.score);
                out[q].VecScores.push_back(f.vec_score);
                out[q].LexRanks.push_back(f.lex_rank);
                out[q].VecRanks.push_back(f.vec_rank);
            }
        }
        return out;
    }

    // On-disk snapshot of the flattened tables with the md5-hex <-> dense-id maps: written once after
    // the offline rank update, read at every server start instead of decoding the JSON tables.
    void save_snapshot(const std::string& path) { sync_flat(); flat.save(path); }
    void load_snapshot(const std::string& path) {
        flat.load(path);
        docs.name = flat.doc_names;
        terms.name = flat.term_names;
        docs.id.clear();
        terms.id.clear();
        for (size_t i = 0; i < docs.name.size(); i++) docs.id[docs.name[i]] = (uint32_t)i;
        for (size_t i = 0; i < terms.name.size(); i++) terms.id[terms.name[i]] = (uint32_t)i;
        upload();
    }

    // ---- incremental re-index of one page on the resident tables --------------------------------------
    // The table side repeats the reference's writes: checkAndUpdate removes the page's old title words from inv[0]
    // (indexer.go:455-492), its old body words from inv[1] (:494-531) and the postings its anchor words made in its old
    // children's title rows (:533-616; the child's WHOLE posting of that word goes, also what other parents put there);
    // the re-index upserts the new postings (`value[docHash] = ...`, :395-403 and :277-285) and rewrites forw[2] (:301-304).
    // [The reference collects these writes in batch writers fed from reads of the pre-state, so of two removals that hit
    // the same row only the last (in goroutine order) survives the flush; here every removal is applied.]
    // The device side is ONE delta per table: pairs to delete, postings to add (an upsert deletes its pair first), merged
    // into the resident CSR by ss_index_apply_delta_pos after growing the doc / term space for new children and new words.
    // Weights are stored as given (listPos[0]).  update_magnitudes: the touched docs' magnitudes follow the delta on the
    // device (O(delta) once the squared magnitudes are resident) and their forw[4] rows are rewritten; false leaves
    // forw[4] and the device magnitudes as they were, which is what the reference serves until the next UpdateTermWeights.
    void ApplyDelta(db::Context& ctx, std::vector<db::DB*>& forw, std::vector<db::DB*>& inv, const PageIndexInfo& before,
                    const PageIndexInfo& after, bool update_magnitudes = true) {
        using namespace spaghetti;
        if (!title || !body) throw std::runtime_error("ApplyDelta: the index is not loaded");
        if (before.docHash != after.docHash) throw std::runtime_error("ApplyDelta: before and after describe different pages");
        struct Post { std::string term, doc; std::vector<float> listPos; };
        std::vector<std::pair<std::string, std::string>> del[2];          // (wordHash, docHash) per table
        std::vector<Post> add[2];
        for (auto& kv : before.title) del[0].emplace_back(kv.first, before.docHash);
        for (auto& kv : before.body) del[1].emplace_back(kv.first, before.docHash);
        for (auto& ch : before.anchors)
            for (auto& kv : ch.second) del[0].emplace_back(kv.first, ch.first);
        for (auto& kv : after.title) add[0].push_back({kv.first, after.docHash, kv.second});
        for (auto& kv : after.body) add[1].push_back({kv.first, after.docHash, kv.second});
        for (auto& ch : after.anchors)
            for (auto& kv : ch.second) add[0].push_back({kv.first, ch.first, kv.second});
        for (int t = 0; t < 2; t++)
            for (auto& a : add[t])
                if (a.listPos.empty()) throw std::runtime_error("ApplyDelta: posting without a weight entry");
        // --- device -----------------------------------------------------------------------------------------------------
        auto grow = [](DenseIds& ids, const std::string& h) {
            auto it = ids.id.find(h);
            if (it != ids.id.end()) return it->second;
            const uint32_t v = (uint32_t)ids.name.size();
            ids.name.push_back(h);
            ids.id[h] = v;
            return v;
        };
        // The device goes FIRST and the tables follow only once both resident tables have taken their delta: a failing
        // library call must not leave inv[] / forw[2] ahead of the index that answers queries.  Whatever happens, the index
        // stays servable: the scorer is re-created on every way out (ScorerGuard), and ids grown for a delta that did not
        // happen are taken back while the device tables still have their old size.
        const size_t n_before = docs.name.size(), t_before = terms.name.size();
        for (int t = 0; t < 2; t++)
            for (auto& a : add[t]) { grow(docs, a.doc); grow(terms, a.term); }
        for (auto& c : after.children) grow(docs, c);
        const size_t n = docs.name.size(), T = terms.name.size();
        struct ScorerGuard {
            DeviceIndex& di;
            ~ScorerGuard() {
                if (di.scorer || !di.title || !di.body) return;
                const size_t K = di.categories.size(), nd = di.docs.name.size();
                if (ss_scorer_create(spaghetti::default_ctx(), di.title, di.body, &di.scorer) != SS_OK) { di.scorer = nullptr; return; }
                if (K > 0 && K <= SS_MAX_TOPICS && di.flat.prior.size() == K * nd) (void)ss_scorer_set_prior(di.scorer, (int32_t)K, di.flat.prior.data());
                try { di.register_masks(); } catch (...) { di.mask_index.clear(); }
                try { di.register_groups(); } catch (...) {}                // (RetrieveBatchCollapsed then reports the missing table)
                try { di.register_fields(); } catch (...) {}                // (RetrieveBatchFiltered then reports the missing table)
                try { di.register_vectors(); } catch (...) {}               // (VectorSearch then reports the missing table)
                try { di.register_tokens(); } catch (...) {}                // (RerankByMaxSim then reports the missing table)
                try { di.build_doc_view(); } catch (...) {}                 // (SimilarPages then reports the missing view)
                try { di.build_signatures(); } catch (...) {}               // (RetrieveBatchDeduped then reports the missing signatures)
            }
        } scorer_guard{*this};
        bool resized = false;
        auto shrink_ids = [&] {
            if (resized) return;                                          // the device tables hold the new ids (as empty docs / terms)
            for (size_t v = n_before; v < docs.name.size(); v++) docs.id.erase(docs.name[v]);
            docs.name.resize(n_before);
            for (size_t v = t_before; v < terms.name.size(); v++) terms.id.erase(terms.name[v]);
            terms.name.resize(t_before);
        };
        if (scorer) { ss_scorer_destroy(scorer); scorer = nullptr; }      // scorers on a table go before its delta
        doc_view_built = signatures_built = false;                        // resize / the delta free the view and the signatures; every way out builds them again
        try {
            if (n != n_before || T != t_before) {
                check(ss_index_resize(title, n, T), "ss_index_resize(title)");
                resized = true;
                check(ss_index_resize(body, n, T), "ss_index_resize(body)");
            }
        } catch (...) {
            if (resized) (void)ss_index_resize(body, n, T);               // title grew: body must follow or the ids diverge
            shrink_ids();
            throw;
        }
        // the PageRank table follows the doc space at once (the guard's scorer needs a table of the new size): new docs hold 0
        // until the next PageRank run (ReloadPrior)
        if (n != n_before && !categories.empty()) {
            const size_t K = categories.size();
            std::vector<double> grown(K * n, 0.0);
            for (size_t k = 0; k < K; k++) std::copy(flat.prior.begin() + k * n_before, flat.prior.begin() + (k + 1) * n_before, grown.begin() + k * n);
            flat.prior.swap(grown);
        }
        if (update_magnitudes && !mags_resident) {                        // once: squared magnitudes of the stored weights
            check(ss_index_refresh_magnitudes(title, nullptr), "ss_index_refresh_magnitudes(title)");
            check(ss_index_refresh_magnitudes(body, nullptr), "ss_index_refresh_magnitudes(body)");
            mags_resident = true;
        }
        std::vector<uint32_t> touched;
        ss_index* table[2] = {title, body};
        for (int t = 0; t < 2; t++) {
            std::vector<uint32_t> del_term, del_doc, add_term, add_doc;
            std::vector<float> add_w, add_pos;
            std::vector<uint64_t> add_pos_ptr{0};
            std::map<std::pair<uint32_t, uint32_t>, bool> seen;
            auto del_pair = [&](const std::string& w, const std::string& d) {
                auto ti = terms.id.find(w);
                auto di = docs.id.find(d);
                if (ti == terms.id.end() || di == docs.id.end()) return;  // never indexed: nothing to delete
                if (seen.emplace(std::make_pair(ti->second, di->second), true).second) {
                    del_term.push_back(ti->second);
                    del_doc.push_back(di->second);
                    touched.push_back(di->second);
                }
            };
            for (auto& d : del[t]) del_pair(d.first, d.second);
            for (auto& a : add[t]) del_pair(a.term, a.doc);               // upsert
            std::map<std::pair<uint32_t, uint32_t>, const Post*> last;    // the last write of a (word, doc) wins, as in a map
            for (auto& a : add[t]) last[{terms.id[a.term], docs.id[a.doc]}] = &a;
            for (auto& kv : last) {
                add_term.push_back(kv.first.first);
                add_doc.push_back(kv.first.second);
                add_w.push_back(kv.second->listPos[0]);
                add_pos.insert(add_pos.end(), kv.second->listPos.begin() + 1, kv.second->listPos.end());
                add_pos_ptr.push_back(add_pos.size());
                touched.push_back(kv.first.second);
            }
            const int32_t rc = ss_index_apply_delta_pos(table[t], 0, nullptr, del_term.size(), del_term.data(), del_doc.data(), add_term.size(),
                                                        add_term.data(), add_doc.data(), add_w.data(), add_pos_ptr.data(), add_pos.data());
            if (rc != SS_OK) {
                flat_stale = true;
                const std::string why = ss_last_error(default_ctx());
                if (t == 0) { shrink_ids(); throw std::runtime_error("ss_index_apply_delta_pos(title): " + why + " (nothing changed)"); }
                throw std::runtime_error("ss_index_apply_delta_pos(body): " + why + " — the resident title table already holds its delta and the tables do not: load() again");
            }
        }
        // --- tables (the device has taken both deltas) -----------------------------------------------------------------------------------------------------
        for (int t = 0; t < 2; t++) {
            std::map<std::string, std::map<std::string, std::vector<float>>> rows;   // the rows this delta touches
            auto row_of = [&](const std::string& w) -> std::map<std::string, std::vector<float>>& {
                auto it = rows.find(w);
                if (it != rows.end()) return it->second;
                auto& r = rows[w];
                if (inv[t]->Has(ctx, w)) r = jsonmini::parse_map_f32list(inv[t]->Get(ctx, w));
                return r;
            };
            for (auto& d : del[t]) row_of(d.first).erase(d.second);
            for (auto& a : add[t]) row_of(a.term)[a.doc] = a.listPos;
            auto bw = inv[t]->BatchWrite_init(ctx);
            for (auto& r : rows) {
                if (r.second.empty()) { if (inv[t]->Has(ctx, r.first)) inv[t]->Delete(ctx, r.first); }   // "delete this row" (:484-489)
                else bw->BatchSet(ctx, r.first, jsonmini::dump(r.second));
            }
            bw->Flush(ctx);
        }
        forw[2]->Set(ctx, after.docHash, jsonmini::dump(after.children));

        std::sort(touched.begin(), touched.end());
        touched.erase(std::unique(touched.begin(), touched.end()), touched.end());
        if (update_magnitudes && !touched.empty()) {
            std::vector<double> mt(touched.size()), mb(touched.size());
            check(ss_index_read_magnitudes(title, touched.size(), touched.data(), mt.data()), "ss_index_read_magnitudes(title)");
            check(ss_index_read_magnitudes(body, touched.size(), touched.data(), mb.data()), "ss_index_read_magnitudes(body)");
            auto bw = forw[4]->BatchWrite_init(ctx);
            for (size_t i = 0; i < touched.size(); i++) {
                const std::string& d = docs.name[touched[i]];
                std::map<std::string, double> row;
                if (forw[4]->Has(ctx, d)) row = jsonmini::parse_map_f64(forw[4]->Get(ctx, d));
                row["title"] = mt[i];
                row["body"] = mb[i];
                bw->BatchSet(ctx, d, jsonmini::dump(row));
            }
            bw->Flush(ctx);
        }
        flat_stale = true;
        const size_t K = categories.size();
        check(ss_scorer_create(default_ctx(), title, body, &scorer), "ss_scorer_create");
        if (K > 0 && K <= SS_MAX_TOPICS) check(ss_scorer_set_prior(scorer, (int32_t)K, flat.prior.data()), "ss_scorer_set_prior");
        register_masks();                                                 // the new scorer, the ids as they stand now
        register_groups();
        register_fields();
        register_vectors();
        register_tokens();
        build_doc_view();                                                 // (the deltas freed it)
        build_signatures();
        refresh_lexicon(ctx, forw[0], t_before);                          // new term ids: a new lexicon; otherwise the frequencies only
    }

    // forw[3] was rewritten (UpdateTopicSensitivePagerank / ResidentPagerank::Run): refresh the scorer's PageRank table.
    void ReloadPrior(db::Context& ctx, std::vector<db::DB*>& forw) {
        using namespace spaghetti;
        const std::vector<db::KV> ranks = forw[3]->Iterate(ctx);
        std::vector<std::string> cat;
        for (auto& kv : ranks) for (auto& c : jsonmini::parse_map_f64(kv.second)) cat.push_back(c.first);
        std::sort(cat.begin(), cat.end());
        cat.erase(std::unique(cat.begin(), cat.end()), cat.end());
        const size_t K = cat.size(), n = docs.name.size();
        flat.categories = categories = cat;
        flat.prior.assign(K * n, 0.0);
        for (auto& kv : ranks) {
            auto it = docs.id.find(kv.first);
            if (it == docs.id.end()) continue;                 // a node that is in no table yet: cannot be retrieved either
            for (auto& c : jsonmini::parse_map_f64(kv.second))
                flat.prior[(std::lower_bound(cat.begin(), cat.end(), c.first) - cat.begin()) * n + it->second] = c.second;
        }
        if (scorer) check(ss_scorer_set_prior(scorer, K <= SS_MAX_TOPICS ? (int32_t)K : 0, flat.prior.data()), "ss_scorer_set_prior");
    }

    // after deltas the flattened host copy is read back from the device (only save_snapshot needs it)
    void sync_flat() {
        using namespace spaghetti;
        if (!flat_stale) return;
        const size_t n = docs.name.size();
        flat.doc_names = docs.name;
        flat.term_names = terms.name;
        ss_index* table[2] = {title, body};
        FlatTable* ft[2] = {&flat.title, &flat.body};
        for (int t = 0; t < 2; t++) {
            uint64_t nd = 0, nt = 0, np = 0;
            check(ss_index_get_info(table[t], &nd, &nt, &np), "ss_index_get_info");
            ft[t]->term_ptr.resize(nt + 1);
            ft[t]->post_doc.resize(np);
            ft[t]->post_w.resize(np);
            check(ss_index_read(table[t], ft[t]->term_ptr.data(), ft[t]->post_doc.data(), ft[t]->post_w.data()), "ss_index_read");
            ft[t]->pos_ptr.resize(np + 1);
            check(ss_index_read_positions(table[t], ft[t]->pos_ptr.data(), nullptr), "ss_index_read_positions");
            ft[t]->pos.resize(ft[t]->pos_ptr[np]);
            check(ss_index_read_positions(table[t], nullptr, ft[t]->pos.data()), "ss_index_read_positions");
            std::vector<uint32_t> all(n);
            for (size_t i = 0; i < n; i++) all[i] = (uint32_t)i;
            ft[t]->mag.resize(n);
            check(ss_index_read_magnitudes(table[t], n, all.data(), ft[t]->mag.data()), "ss_index_read_magnitudes");
        }
        flat_stale = false;
    }

    // OPT-IN: the ODP keyword vectors for computeTopicProbs at query time — the call the reference has
    // commented out (main_retrieve.go:41-43,87-88).  Kept as hash maps in host memory: a query has a handful of words.
    std::unordered_map<std::string, std::vector<std::pair<uint32_t, double>>> keyword_topics;   // wordHash -> (index into topic_names, frequency)
    std::vector<std::string> topic_names;                                                       // forw[5] keys
    std::vector<double> topic_word_count;
    void LoadTopics(db::Context& ctx, std::vector<db::DB*>& forw, std::vector<db::DB*>& inv) {
        topic_names.clear();
        topic_word_count.clear();
        keyword_topics.clear();
        for (auto& kv : forw[5]->Iterate(ctx)) {
            auto md = jsonmini::parse_map_f64(kv.second);
            topic_names.push_back(kv.first);
            topic_word_count.push_back(md.count("wordCount") ? md["wordCount"] : 0.0);
        }
        for (auto& kv : inv[2]->Iterate(ctx)) {
            auto& v = keyword_topics[kv.first];
            for (auto& tf : jsonmini::parse_map_f64(kv.second)) {
                auto it = std::lower_bound(topic_names.begin(), topic_names.end(), tf.first);
                if (it != topic_names.end() && *it == tf.first) v.emplace_back((uint32_t)(it - topic_names.begin()), tf.second);
            }
        }
    }
    // computeTopicProbs (main_retrieve.go:106-159) with the product started at 1 (as_written = false above), on the
    // resident keyword vectors.  A query word outside inv[2] carries no topic information and is skipped — the reference
    // would panic on it (:120-121), which no serving path can afford.
    std::map<std::string, double> liveTopicProbs(const std::vector<std::string>& queryTokenised) const {
        const size_t K = topic_names.size();
        std::vector<double> probs(K, 1.0);
        std::vector<char> seen(K, 0);
        for (auto& tok : queryTokenised) {
            auto it = keyword_topics.find(tok);
            if (it == keyword_topics.end()) continue;
            for (auto& cf : it->second) { probs[cf.first] *= cf.second / topic_word_count[cf.first]; seen[cf.first] = 1; }   // :143-145
        }
        std::map<std::string, double> out;
        for (size_t c = 0; c < K; c++) out[topic_names[c]] = seen[c] ? probs[c] / (double)K : 0.0;                            // :148,:150
        return out;
    }

    // A batch of queries in one library call (additive API).  topicProbs: per query
    // category -> probability, or empty (nil map in the shipped reference, main_retrieve.go:88: sqd = 0).
    // live_topic_probs (opt-in, default off = the reference's nil map): every query's probabilities come from
    // liveTopicProbs over its non-phrase words (the argument of the commented-out call, main_retrieve.go:43).
    // what a batch of query strings becomes on its way to the device (main_retrieve.go:17-36,88-90)
    struct Tokenised {
        std::vector<uint32_t> q_ptr{0}, q_terms, p_ptr{0}, p_terms;
        std::vector<int32_t> q_len;
        std::vector<double> probs;
        int nq = 0;
    };
    Tokenised tokenise(const std::vector<std::string>& queries, const std::vector<std::map<std::string, double>>* topicProbs,
                       bool live_topic_probs) const {
        using namespace spaghetti;
        Tokenised t;
        std::vector<std::map<std::string, double>> live;
        if (live_topic_probs) {
            if (topicProbs) throw std::runtime_error("RetrieveBatch: explicit and live topic probabilities are exclusive");
            if (topic_names.empty()) throw std::runtime_error("RetrieveBatch: live topic probabilities need LoadTopics");
        }
        // SetPrefixQueries: the "word*" tokens leave the strings, and all of them are completed by ONE ss_lexicon_complete call (the one
        // place the mirror waits for the lexicon); expansion[e] = the term ids of prefix token e, best first
        std::vector<std::string> cut;
        std::vector<uint32_t> pre_ptr{0};                // prefix tokens of the queries before q
        std::vector<std::vector<uint32_t>> expansion;
        if (prefix_expansions > 0) {
            std::vector<uint32_t> p_ptr{0};
            std::string p_bytes;
            for (auto& q : queries) {
                PrefixTokens pt = parsePrefixTokens(q, query_operators, laundry);
                cut.push_back(pt.query);
                for (auto& pre : pt.prefixes) {
                    p_bytes += pre;
                    p_ptr.push_back((uint32_t)p_bytes.size());
                }
                pre_ptr.push_back((uint32_t)(p_ptr.size() - 1));
            }
            const size_t np = p_ptr.size() - 1, m = (size_t)prefix_expansions;
            if (np) {
                if (!lexicon) throw std::runtime_error("RetrieveBatch: prefix queries need the lexicon (SetLexicon)");
                std::vector<uint32_t> ids(np * m);
                std::vector<int32_t> n(np);
                check(ss_lexicon_complete(lexicon, (int32_t)np, p_ptr.data(), reinterpret_cast<const uint8_t*>(p_bytes.data()), 1u,
                                          prefix_expansions, ids.data(), nullptr, n.data(), nullptr), "ss_lexicon_complete");
                expansion.resize(np);
                for (size_t e = 0; e < np; e++) expansion[e].assign(ids.begin() + e * m, ids.begin() + e * m + n[e]);
            }
        }
        for (size_t qn = 0; qn < queries.size(); qn++) {
            std::string query = cut.empty() ? queries[qn] : cut[qn];
            // main_retrieve.go:17-36
            const std::vector<std::string> phrases = getPhrase(query);
            for (auto& ph : phrases) {
                const size_t pos = query.find("\"" + ph + "\"");
                if (pos != std::string::npos) query.erase(pos, ph.size() + 2);
            }
            std::string joined;
            for (auto& ph : phrases) joined += ph + " ";
            const std::vector<std::string> queryTokenised = laundry(query), phraseTokenised = laundry(joined);
            std::vector<std::string> hashed;
            for (auto& tok : queryTokenised) {
                hashed.push_back(md5::hex(tok));
                auto it = terms.id.find(hashed.back());
                t.q_terms.push_back(it == terms.id.end() ? SS_UNKNOWN_TERM : it->second);   // ErrKeyNotFound tolerated (:193,:218)
            }
            if (live_topic_probs) live.push_back(liveTopicProbs(hashed));
            // the completions of the query's prefix tokens, as plain OR terms behind its words: in the order the tokens stand, each
            // list best first, a token without a completion as one unknown word; what would take the query past SS_MAX_QUERY_TERMS
            // is dropped
            const size_t n_pre = cut.empty() ? 0 : pre_ptr[qn + 1] - pre_ptr[qn];
            for (size_t e = 0; e < n_pre; e++) {
                const std::vector<uint32_t>& ids = expansion[pre_ptr[qn] + e];
                const size_t room = (size_t)SS_MAX_QUERY_TERMS - std::min<size_t>(SS_MAX_QUERY_TERMS, t.q_terms.size() - t.q_ptr.back());
                if (ids.empty() && room) t.q_terms.push_back(SS_UNKNOWN_TERM);
                t.q_terms.insert(t.q_terms.end(), ids.begin(), ids.begin() + std::min(room, ids.size()));
            }
            t.q_ptr.push_back((uint32_t)t.q_terms.size());
            // all quoted phrases form ONE phrase (main_retrieve.go:26), matched on the device (retrieval/phrase.go)
            for (auto& tok : phraseTokenised) {
                auto it = terms.id.find(md5::hex(tok));
                t.p_terms.push_back(it == terms.id.end() ? SS_UNKNOWN_TERM : it->second);
            }
            t.p_ptr.push_back((uint32_t)t.p_terms.size());
            t.q_len.push_back((int32_t)(queryTokenised.size() + phraseTokenised.size() + n_pre));   // :90 (a prefix token is one typed word)
        }
        t.nq = (int)queries.size();
        const size_t K = categories.size();
        if (live_topic_probs) topicProbs = &live;
        if (topicProbs && K) {
            t.probs.assign((size_t)t.nq * K, 0.0);
            for (int q = 0; q < t.nq; q++)
                for (auto& kv : (*topicProbs)[q]) {
                    auto it = std::lower_bound(categories.begin(), categories.end(), kv.first);
                    if (it != categories.end() && *it == kv.first) t.probs[(size_t)q * K + (it - categories.begin())] = kv.second;
                }
        }
        return t;
    }
    std::vector<std::vector<Rank_combined>> to_ranks(int nq, int k, const std::vector<ss_hit>& hits, const std::vector<int32_t>& n_hits) const {
        std::vector<std::vector<Rank_combined>> out(nq);
        for (int q = 0; q < nq; q++)
            for (int i = 0; i < n_hits[q]; i++) {
                const auto& h = hits[(size_t)q * k + i];
                Rank_combined r;
                r.DocHash = docs.name[h.doc];
                r.PageRank = h.pagerank;      // get_metadata.go:68
                r.FinalRank = h.final;        // get_metadata.go:69
                r.TitleRank = h.title;
                r.BodyRank = h.body;
                out[q].push_back(r);
            }
        return out;
    }
    // Query operators on (default off): RetrieveBatch reads "+word" / "-word" (parseQueryOperators) and answers through
    // ss_score_topk_constrained.  Off, every query string is tokenised as it always was, '+' and '-' included.
    void SetQueryOperators(bool on) { query_operators = on; }
    // RetrieveBatch with query operators: mask_id as for ss_score_topk_masked (NULL: none)
    std::vector<std::vector<Rank_combined>> retrieve_constrained(const std::vector<std::string>& queries, const int32_t* mask_id, int k,
                                                                 const std::vector<std::map<std::string, double>>* topicProbs,
                                                                 bool live_topic_probs) {
        using namespace spaghetti;
        std::vector<std::string> rewritten;
        std::vector<uint32_t> req_ptr{0}, req_terms, exc_ptr{0}, exc_terms;
        auto id_of = [&](const std::string& w) {
            auto it = terms.id.find(md5::hex(w));
            return it == terms.id.end() ? SS_UNKNOWN_TERM : it->second;
        };
        for (auto& q : queries) {
            const QueryOperators op = parseQueryOperators(q, laundry);
            rewritten.push_back(op.query);
            for (auto& w : op.required) req_terms.push_back(id_of(w));
            for (auto& w : op.excluded) exc_terms.push_back(id_of(w));
            req_ptr.push_back((uint32_t)req_terms.size());
            exc_ptr.push_back((uint32_t)exc_terms.size());
        }
        const Tokenised t = tokenise(rewritten, topicProbs, live_topic_probs);
        std::vector<ss_hit> hits((size_t)t.nq * k);
        std::vector<int32_t> n_hits(t.nq);
        check(ss_score_topk_constrained(scorer, t.nq, t.q_ptr.data(), t.q_terms.data(), t.p_ptr.data(), t.p_terms.data(), t.q_len.data(),
                                        t.probs.empty() ? nullptr : t.probs.data(), mask_id, req_ptr.data(), req_terms.data(),
                                        exc_ptr.data(), exc_terms.data(), k, hits.data(), n_hits.data()),
              "ss_score_topk_constrained");
        return to_ranks(t.nq, k, hits, n_hits);
    }
    std::vector<std::vector<Rank_combined>> RetrieveBatch(const std::vector<std::string>& queries, int k = 50,
                                                          const std::vector<std::map<std::string, double>>* topicProbs = nullptr,
                                                          bool live_topic_probs = false) {
        using namespace spaghetti;
        if (query_operators) return retrieve_constrained(queries, nullptr, k, topicProbs, live_topic_probs);
        const Tokenised t = tokenise(queries, topicProbs, live_topic_probs);
        std::vector<ss_hit> hits((size_t)t.nq * k);
        std::vector<int32_t> n_hits(t.nq);
        check(ss_score_topk_phrase(scorer, t.nq, t.q_ptr.data(), t.q_terms.data(), t.p_ptr.data(), t.p_terms.data(), t.q_len.data(),
                                   t.probs.empty() ? nullptr : t.probs.data(), k, hits.data(), n_hits.data()), "ss_score_topk_phrase");
        return to_ranks(t.nq, k, hits, n_hits);
    }
    // RetrieveBatch with one allow-list per query: masks[q] names a set of SetDocMasks, "" = the whole index.  Row q holds
    // the first k docs of query q's ranking that the set allows (not a filter of the unrestricted top k).
    std::vector<std::vector<Rank_combined>> RetrieveBatch(const std::vector<std::string>& queries, const std::vector<std::string>& masks,
                                                          int k = 50, const std::vector<std::map<std::string, double>>* topicProbs = nullptr,
                                                          bool live_topic_probs = false) {
        using namespace spaghetti;
        if (masks.size() != queries.size()) throw std::runtime_error("RetrieveBatch: one mask name per query");
        std::vector<int32_t> mask_id(queries.size(), -1);
        for (size_t q = 0; q < masks.size(); q++) {
            if (masks[q].empty()) continue;
            auto it = mask_index.find(masks[q]);
            if (it == mask_index.end()) throw std::runtime_error("RetrieveBatch: no doc mask named '" + masks[q] + "' (SetDocMasks)");
            mask_id[q] = it->second;
        }
        if (query_operators) return retrieve_constrained(queries, mask_id.data(), k, topicProbs, live_topic_probs);
        const Tokenised t = tokenise(queries, topicProbs, live_topic_probs);
        std::vector<ss_hit> hits((size_t)t.nq * k);
        std::vector<int32_t> n_hits(t.nq);
        check(ss_score_topk_masked(scorer, t.nq, t.q_ptr.data(), t.q_terms.data(), t.p_ptr.data(), t.p_terms.data(), t.q_len.data(),
                                   t.probs.empty() ? nullptr : t.probs.data(), mask_id.data(), k, hits.data(), n_hits.data()),
              "ss_score_topk_masked");
        return to_ranks(t.nq, k, hits, n_hits);
    }
    // RetrieveBatch with at most g rows per site (SetDocGroups): page [first, first + k) of every query's ranking after the
    // collapse, taken over the first k_window rows of the ranking (a window that comes back full can continue past its end: ask with
    // a larger window for deeper pages; k_window <= SS_MAX_TOPK).  Queries without quoted phrases are scored and collapsed in one
    // library call and only the pages come back (ss_score_topk_collapsed); a batch with a quoted phrase is scored by
    // ss_score_topk_phrase and its rows go through ss_collapse_hits.  Query operators are not read here.
    std::vector<CollapsedPage> RetrieveBatchCollapsed(const std::vector<std::string>& queries, int k_window, int g, int first = 0,
                                                      int k = 50, const std::vector<std::map<std::string, double>>* topicProbs = nullptr,
                                                      bool live_topic_probs = false) {
        using namespace spaghetti;
        if (!has_doc_groups) throw std::runtime_error("RetrieveBatchCollapsed: no site keys (SetDocGroups)");
        if (query_operators) throw std::runtime_error("RetrieveBatchCollapsed: query operators are not read here (SetQueryOperators(false))");
        if (prefix_expansions) throw std::runtime_error("RetrieveBatchCollapsed: prefix queries are not read here (SetPrefixQueries(0))");
        const Tokenised t = tokenise(queries, topicProbs, live_topic_probs);
        const size_t nq = (size_t)t.nq, kk = (size_t)std::max(k, 1);
        std::vector<ss_hit> page(nq * kk);
        std::vector<int32_t> n_page(nq), n_kept(nq);
        std::vector<uint32_t> same(nq * kk);
        const double* probs = t.probs.empty() ? nullptr : t.probs.data();
        if (t.p_terms.empty()) {
            check(ss_score_topk_collapsed(scorer, t.nq, t.q_ptr.data(), t.q_terms.data(), t.q_len.data(), probs, nullptr, k_window, g, first, k,
                                          page.data(), n_page.data(), same.data(), n_kept.data()), "ss_score_topk_collapsed");
        } else {
            std::vector<ss_hit> rows(nq * (size_t)std::max(k_window, 1));
            std::vector<int32_t> n_rows(nq);
            check(ss_score_topk_phrase(scorer, t.nq, t.q_ptr.data(), t.q_terms.data(), t.p_ptr.data(), t.p_terms.data(), t.q_len.data(), probs,
                                       k_window, rows.data(), n_rows.data()), "ss_score_topk_phrase");
            check(ss_collapse_hits(scorer, t.nq, k_window, rows.data(), n_rows.data(), g, first, k, page.data(), n_page.data(), same.data(),
                                   n_kept.data()), "ss_collapse_hits");
        }
        const std::vector<std::vector<Rank_combined>> ranks = to_ranks(t.nq, k, page, n_page);
        std::vector<CollapsedPage> out(nq);
        for (size_t q = 0; q < nq; q++) {
            out[q].Results = ranks[q];
            out[q].Same.assign(same.begin() + q * kk, same.begin() + q * kk + n_page[q]);
            out[q].Kept = n_kept[q];
        }
        return out;
    }
    // RetrieveBatch re-ranked by term proximity: page [first, first + k) of every query's first k_window rows, sorted by
    // w_rank * FinalRank + w_prox * bonus (bonus: how close the query's words come in the page's body, times the share of the query's
    // words the page has; k_window <= SS_MAX_TOPK).  Queries without quoted phrases are scored and re-ranked in one library call and
    // only the pages come back (ss_score_topk_proximity); a batch with a quoted phrase is scored by ss_score_topk_phrase and its rows
    // go through ss_rerank_hits_by_proximity, the phrases' words counting as tokens behind the others.  Query operators and prefix
    // queries are not read here.
    std::vector<ProximityPage> RetrieveBatchProximity(const std::vector<std::string>& queries, int k_window, double w_rank = 1.0,
                                                      double w_prox = 1.0, int first = 0, int k = 50,
                                                      const std::vector<std::map<std::string, double>>* topicProbs = nullptr,
                                                      bool live_topic_probs = false) {
        using namespace spaghetti;
        if (query_operators) throw std::runtime_error("RetrieveBatchProximity: query operators are not read here (SetQueryOperators(false))");
        if (prefix_expansions) throw std::runtime_error("RetrieveBatchProximity: prefix queries are not read here (SetPrefixQueries(0))");
        const Tokenised t = tokenise(queries, topicProbs, live_topic_probs);
        const size_t nq = (size_t)t.nq, kk = (size_t)std::max(k, 1);
        std::vector<ss_hit> page(nq * kk);
        std::vector<int32_t> n_page(nq);
        std::vector<double> scores(nq * kk);
        std::vector<ss_proximity> prox(nq * kk);
        std::vector<uint32_t> w_ptr{0}, w_terms;                 // the re-rank's tokens of a batch with a quoted phrase
        const double* probs = t.probs.empty() ? nullptr : t.probs.data();
        if (t.p_terms.empty()) {
            check(ss_score_topk_proximity(scorer, t.nq, t.q_ptr.data(), t.q_terms.data(), t.q_len.data(), probs, nullptr, k_window, w_rank, w_prox,
                                          first, k, page.data(), n_page.data(), scores.data(), prox.data()), "ss_score_topk_proximity");
        } else {
            std::vector<ss_hit> rows(nq * (size_t)std::max(k_window, 1));
            std::vector<int32_t> n_rows(nq);
            check(ss_score_topk_phrase(scorer, t.nq, t.q_ptr.data(), t.q_terms.data(), t.p_ptr.data(), t.p_terms.data(), t.q_len.data(), probs,
                                       k_window, rows.data(), n_rows.data()), "ss_score_topk_phrase");
            // the words of the quoted phrases count as tokens, behind the others (as query_word_hashes reads a query), up to
            // SS_MAX_QUERY_TERMS
            for (size_t q = 0; q < nq; q++) {
                w_terms.insert(w_terms.end(), t.q_terms.begin() + t.q_ptr[q], t.q_terms.begin() + t.q_ptr[q + 1]);
                for (uint32_t i = t.p_ptr[q]; i < t.p_ptr[q + 1] && w_terms.size() - w_ptr.back() < (size_t)SS_MAX_QUERY_TERMS; i++)
                    w_terms.push_back(t.p_terms[i]);
                w_ptr.push_back((uint32_t)w_terms.size());
            }
            check(ss_rerank_hits_by_proximity(scorer, t.nq, w_ptr.data(), w_terms.data(), k_window, rows.data(), n_rows.data(), w_rank, w_prox,
                                              first, k, page.data(), n_page.data(), scores.data(), prox.data()), "ss_rerank_hits_by_proximity");
        }
        const std::vector<uint32_t>& tok_ptr = t.p_terms.empty() ? t.q_ptr : w_ptr;
        const std::vector<uint32_t>& tok = t.p_terms.empty() ? t.q_terms : w_terms;
        const std::vector<std::vector<Rank_combined>> ranks = to_ranks(t.nq, k, page, n_page);
        std::vector<ProximityPage> out(nq);
        for (size_t q = 0; q < nq; q++) {
            std::vector<std::string> names;
            for (uint32_t i = tok_ptr[q]; i < tok_ptr[q + 1]; i++) names.push_back(tok[i] < terms.name.size() ? terms.name[tok[i]] : std::string());
            out[q].Results = ranks[q];
            out[q].Scores.assign(scores.begin() + q * kk, scores.begin() + q * kk + n_page[q]);
            for (int32_t r = 0; r < n_page[q]; r++) out[q].Spans.push_back(to_proximity(prox[q * kk + r], names));
        }
        return out;
    }
    // The model of RetrieveBatchRanked: linear (empty: none) and base, and the trees as ss_rank_model_create takes them (tree t =
    // nodes [tree_ptr[t], tree_ptr[t + 1]), a node = {feature or -1, left, right, nan_left, value}).  The library validates the whole
    // model; one it refuses leaves the previous model in place.
    using TreeNode = std::tuple<int32_t, uint32_t, uint32_t, uint32_t, double>;
    void SetRankModel(const std::vector<double>& linear, double base, const std::vector<uint32_t>& tree_ptr, const std::vector<TreeNode>& nodes) {
        using namespace spaghetti;
        if (!linear.empty() && linear.size() != (size_t)SS_RANK_N_FEATURES) throw std::runtime_error("SetRankModel: linear holds SS_RANK_N_FEATURES weights or none");
        if (tree_ptr.empty() || tree_ptr.back() != nodes.size()) throw std::runtime_error("SetRankModel: tree_ptr must end at the number of nodes");
        std::vector<ss_tree_node> flat_nodes;
        for (auto& n : nodes) flat_nodes.push_back(ss_tree_node{std::get<0>(n), std::get<1>(n), std::get<2>(n), std::get<3>(n), std::get<4>(n)});
        ss_rank_model* m = nullptr;
        check(ss_rank_model_create(default_ctx(), SS_RANK_N_FEATURES, linear.empty() ? nullptr : linear.data(), base, (int32_t)tree_ptr.size() - 1,
                                   tree_ptr.data(), flat_nodes.data(), &m), "ss_rank_model_create");
        if (rank_model) ss_rank_model_destroy(rank_model);
        rank_model = m;
    }
    // RetrieveBatch re-ranked by the model of SetRankModel: page [first, first + k) of every query's first k_window rows, sorted by the
    // model's score of each row's features (ss_score_topk_masked -> ss_hit_proximity -> ss_rerank_hits_by_model; the vector score column
    // is absent, the field columns are those of SetDocFields, query_len is the tokeniser's).  The proximity entries are over the
    // query's words and the words of its quoted phrases behind them, as RetrieveBatchProximity counts them.  Query operators and prefix
    // queries are not read here.
    std::vector<RankedPage> RetrieveBatchRanked(const std::vector<std::string>& queries, int k_window, int first = 0, int k = 50,
                                                const std::vector<std::map<std::string, double>>* topicProbs = nullptr,
                                                bool live_topic_probs = false) {
        using namespace spaghetti;
        if (!rank_model) throw std::runtime_error("RetrieveBatchRanked: no model (SetRankModel)");
        if (query_operators) throw std::runtime_error("RetrieveBatchRanked: query operators are not read here (SetQueryOperators(false))");
        if (prefix_expansions) throw std::runtime_error("RetrieveBatchRanked: prefix queries are not read here (SetPrefixQueries(0))");
        const Tokenised t = tokenise(queries, topicProbs, live_topic_probs);
        const size_t nq = (size_t)t.nq, kk = (size_t)std::max(k, 1), kw = (size_t)std::max(k_window, 1);
        std::vector<ss_hit> rows(nq * kw), page(nq * kk);
        std::vector<int32_t> n_rows(nq), n_page(nq), mask_id(nq, -1);
        std::vector<double> scores(nq * kk);
        std::vector<ss_proximity> prox(nq * kw);
        check(ss_score_topk_masked(scorer, t.nq, t.q_ptr.data(), t.q_terms.data(), t.p_ptr.data(), t.p_terms.data(), t.q_len.data(),
                                   t.probs.empty() ? nullptr : t.probs.data(), mask_id.data(), k_window, rows.data(), n_rows.data()),
              "ss_score_topk_masked");
        std::vector<uint32_t> w_ptr{0}, w_terms;
        for (size_t q = 0; q < nq; q++) {
            w_terms.insert(w_terms.end(), t.q_terms.begin() + t.q_ptr[q], t.q_terms.begin() + t.q_ptr[q + 1]);
            for (uint32_t i = t.p_ptr[q]; i < t.p_ptr[q + 1] && w_terms.size() - w_ptr.back() < (size_t)SS_MAX_QUERY_TERMS; i++)
                w_terms.push_back(t.p_terms[i]);
            w_ptr.push_back((uint32_t)w_terms.size());
        }
        check(ss_hit_proximity(scorer, t.nq, w_ptr.data(), w_terms.data(), k_window, rows.data(), n_rows.data(), prox.data()), "ss_hit_proximity");
        check(ss_rerank_hits_by_model(scorer, rank_model, t.nq, k_window, rows.data(), n_rows.data(), prox.data(), nullptr, t.q_len.data(), first, k,
                                      page.data(), n_page.data(), scores.data()), "ss_rerank_hits_by_model");
        const std::vector<std::vector<Rank_combined>> ranks = to_ranks(t.nq, k, page, n_page);
        std::vector<RankedPage> out(nq);
        for (size_t q = 0; q < nq; q++) {
            out[q].Results = ranks[q];
            out[q].Scores.assign(scores.begin() + q * kk, scores.begin() + q * kk + n_page[q]);
        }
        return out;
    }
    // RetrieveBatch with range clauses per query over the doc fields (SetDocFields): row q holds the first k docs of query q's ranking
    // that match every clause of ranges[q] (not a filter of the unrestricted top k).  With SetQueryOperators "+word" / "-word" are
    // read as in RetrieveBatch; the query strings carry no range syntax.
    std::vector<std::vector<Rank_combined>> RetrieveBatchFiltered(const std::vector<std::string>& queries,
                                                                  const std::vector<std::vector<FieldRange>>& ranges, int k = 50,
                                                                  const std::vector<std::map<std::string, double>>* topicProbs = nullptr,
                                                                  bool live_topic_probs = false) {
        using namespace spaghetti;
        if (!has_doc_fields) throw std::runtime_error("RetrieveBatchFiltered: no doc fields (SetDocFields)");
        if (ranges.size() != queries.size()) throw std::runtime_error("RetrieveBatchFiltered: one list of ranges per query");
        std::vector<uint32_t> rng_ptr{0}, req_ptr{0}, exc_ptr{0}, req_terms, exc_terms;
        std::vector<ss_doc_range> rng;
        for (auto& rs : ranges) {
            for (auto& r : rs) rng.push_back(ss_doc_range{r.field, 0, r.lo, r.hi});
            rng_ptr.push_back((uint32_t)rng.size());
        }
        std::vector<std::string> rewritten;
        const std::vector<std::string>* qs = &queries;
        if (query_operators) {
            auto id_of = [&](const std::string& w) -> uint32_t {
                auto it = terms.id.find(md5::hex(w));
                return it == terms.id.end() ? SS_UNKNOWN_TERM : it->second;
            };
            for (auto& q : queries) {
                const QueryOperators op = parseQueryOperators(q, laundry);
                rewritten.push_back(op.query);
                for (auto& w : op.required) req_terms.push_back(id_of(w));
                for (auto& w : op.excluded) exc_terms.push_back(id_of(w));
                req_ptr.push_back((uint32_t)req_terms.size());
                exc_ptr.push_back((uint32_t)exc_terms.size());
            }
            qs = &rewritten;
        }
        const Tokenised t = tokenise(*qs, topicProbs, live_topic_probs);
        std::vector<ss_hit> hits((size_t)t.nq * std::max(k, 1));
        std::vector<int32_t> n_hits(t.nq);
        check(ss_score_topk_filtered(scorer, t.nq, t.q_ptr.data(), t.q_terms.data(), t.p_ptr.data(), t.p_terms.data(), t.q_len.data(),
                                     t.probs.empty() ? nullptr : t.probs.data(), nullptr, query_operators ? req_ptr.data() : nullptr,
                                     req_terms.data(), query_operators ? exc_ptr.data() : nullptr, exc_terms.data(), rng_ptr.data(), rng.data(),
                                     k, hits.data(), n_hits.data()), "ss_score_topk_filtered");
        return to_ranks(t.nq, k, hits, n_hits);
    }
    // How many docs every query matches (ss_facet_counts): under the clauses of ranges[q] (an empty `ranges`: none for any query), in
    // every set of SetDocMasks, and in every bucket of `buckets` (shared by the batch; needs SetDocFields like a range clause).  The
    // numbers are those of the docs RetrieveBatchFiltered ranks, not of the k it returns.  With SetQueryOperators "+word" / "-word" are
    // read as in RetrieveBatchFiltered.  Quoted phrases are not counted: a query string with one is refused.
    std::vector<FacetCount> FacetCounts(const std::vector<std::string>& queries, const std::vector<std::vector<FieldRange>>& ranges = {},
                                        const std::vector<FieldRange>& buckets = {}) {
        using namespace spaghetti;
        if (!ranges.empty() && ranges.size() != queries.size()) throw std::runtime_error("FacetCounts: one list of ranges per query, or none");
        std::vector<uint32_t> rng_ptr{0}, req_ptr{0}, exc_ptr{0}, req_terms, exc_terms;
        std::vector<ss_doc_range> rng, bk;
        for (auto& rs : ranges) {
            for (auto& r : rs) rng.push_back(ss_doc_range{r.field, 0, r.lo, r.hi});
            rng_ptr.push_back((uint32_t)rng.size());
        }
        for (auto& b : buckets) bk.push_back(ss_doc_range{b.field, 0, b.lo, b.hi});
        if ((!rng.empty() || !bk.empty()) && !has_doc_fields) throw std::runtime_error("FacetCounts: no doc fields (SetDocFields)");
        std::vector<std::string> rewritten;
        const std::vector<std::string>* qs = &queries;
        if (query_operators) {
            auto id_of = [&](const std::string& w) -> uint32_t {
                auto it = terms.id.find(md5::hex(w));
                return it == terms.id.end() ? SS_UNKNOWN_TERM : it->second;
            };
            for (auto& q : queries) {
                const QueryOperators op = parseQueryOperators(q, laundry);
                rewritten.push_back(op.query);
                for (auto& w : op.required) req_terms.push_back(id_of(w));
                for (auto& w : op.excluded) exc_terms.push_back(id_of(w));
                req_ptr.push_back((uint32_t)req_terms.size());
                exc_ptr.push_back((uint32_t)exc_terms.size());
            }
            qs = &rewritten;
        }
        const Tokenised t = tokenise(*qs, nullptr, false);
        if (!t.p_terms.empty()) throw std::runtime_error("FacetCounts: quoted phrases are not counted");
        const size_t n_masks = mask_index.size(), n_b = bk.size();
        std::vector<uint32_t> total(t.nq), by_mask((size_t)t.nq * n_masks), by_bucket((size_t)t.nq * n_b);
        check(ss_facet_counts(scorer, t.nq, t.q_ptr.data(), t.q_terms.data(), nullptr, query_operators ? req_ptr.data() : nullptr, req_terms.data(),
                              query_operators ? exc_ptr.data() : nullptr, exc_terms.data(), ranges.empty() ? nullptr : rng_ptr.data(), rng.data(),
                              (int32_t)n_b, n_b ? bk.data() : nullptr, total.data(), n_masks ? by_mask.data() : nullptr,
                              n_b ? by_bucket.data() : nullptr), "ss_facet_counts");
        std::vector<FacetCount> out(t.nq);
        for (int q = 0; q < t.nq; q++) {
            out[q].Total = total[q];
            for (auto& kv : mask_index) out[q].Masks[kv.first] = by_mask[(size_t)q * n_masks + kv.second];
            out[q].Buckets.assign(by_bucket.begin() + (size_t)q * n_b, by_bucket.begin() + (size_t)(q + 1) * n_b);
        }
        return out;
    }
    // The docs every query matches, ordered by a doc field over ALL matches, not over a relevance window (ss_field_topk): page
    // [first, first + k) of the docs FacetCounts counts under the clauses of ranges[q] (an empty `ranges`: none for any query), by the
    // field's value ascending or descending ("newest first": field 0, descending), equal values by ascending doc hash; first + k <=
    // SS_MAX_TOPK.  Every row is the one the query's ranking holds for that doc (ss_score_docs) with the field's value beside it.  With
    // SetQueryOperators "+word" / "-word" are read as in FacetCounts.  A query string with a quoted phrase is refused.  The host layer
    // holds no device memory of its own: both calls go through the scorer's blocks.
    std::vector<FieldSortedPage> RetrieveBatchByField(const std::vector<std::string>& queries, const std::vector<std::vector<FieldRange>>& ranges,
                                                      int field, bool descending, int first = 0, int k = 50) {
        using namespace spaghetti;
        if (!has_doc_fields) throw std::runtime_error("RetrieveBatchByField: no doc fields (SetDocFields)");
        if (!ranges.empty() && ranges.size() != queries.size()) throw std::runtime_error("RetrieveBatchByField: one list of ranges per query, or none");
        std::vector<uint32_t> rng_ptr{0}, req_ptr{0}, exc_ptr{0}, req_terms, exc_terms;
        std::vector<ss_doc_range> rng;
        for (auto& rs : ranges) {
            for (auto& r : rs) rng.push_back(ss_doc_range{r.field, 0, r.lo, r.hi});
            rng_ptr.push_back((uint32_t)rng.size());
        }
        std::vector<std::string> rewritten;
        const std::vector<std::string>* qs = &queries;
        if (query_operators) {
            auto id_of = [&](const std::string& w) -> uint32_t {
                auto it = terms.id.find(md5::hex(w));
                return it == terms.id.end() ? SS_UNKNOWN_TERM : it->second;
            };
            for (auto& q : queries) {
                const QueryOperators op = parseQueryOperators(q, laundry);
                rewritten.push_back(op.query);
                for (auto& w : op.required) req_terms.push_back(id_of(w));
                for (auto& w : op.excluded) exc_terms.push_back(id_of(w));
                req_ptr.push_back((uint32_t)req_terms.size());
                exc_ptr.push_back((uint32_t)exc_terms.size());
            }
            qs = &rewritten;
        }
        const Tokenised t = tokenise(*qs, nullptr, false);
        if (!t.p_terms.empty()) throw std::runtime_error("RetrieveBatchByField: quoted phrases are not read here");
        const size_t nq = (size_t)t.nq, kk = (size_t)std::max(k, 1);
        std::vector<uint32_t> ids(nq * kk);
        std::vector<int32_t> n_page(nq);
        std::vector<int64_t> values(nq * kk);
        std::vector<ss_hit> page(nq * kk);
        check(ss_field_topk(scorer, t.nq, t.q_ptr.data(), t.q_terms.data(), nullptr, query_operators ? req_ptr.data() : nullptr, req_terms.data(),
                            query_operators ? exc_ptr.data() : nullptr, exc_terms.data(), ranges.empty() ? nullptr : rng_ptr.data(), rng.data(),
                            field, descending ? 1 : 0, first, k, ids.data(), n_page.data(), values.data(), nullptr), "ss_field_topk");
        check(ss_score_docs(scorer, t.nq, t.q_ptr.data(), t.q_terms.data(), t.q_len.data(), nullptr, k, ids.data(), n_page.data(), page.data()),
              "ss_score_docs");
        const std::vector<std::vector<Rank_combined>> ranks = to_ranks(t.nq, k, page, n_page);
        std::vector<FieldSortedPage> out(nq);
        for (size_t q = 0; q < nq; q++) {
            out[q].Results = ranks[q];
            out[q].Values.assign(values.begin() + q * kk, values.begin() + q * kk + n_page[q]);
        }
        return out;
    }
    // Where every query's matches are (ss_top_groups): page [first, first + m) of the site keys of SetDocGroups that hold docs FacetCounts
    // counts under the clauses of ranges[q] (an empty `ranges`: none for any query), by the number of such docs descending, equal counts
    // by ascending key (a key's number is its rank among the distinct keys, so number order is key order); first + m <= SS_MAX_TOPK.
    // With SetQueryOperators "+word" / "-word" are read as in FacetCounts.  A query string with a quoted phrase is refused.
    std::vector<GroupPage> TopGroups(const std::vector<std::string>& queries, const std::vector<std::vector<FieldRange>>& ranges = {}, int first = 0,
                                     int m = 10) {
        using namespace spaghetti;
        if (!has_doc_groups) throw std::runtime_error("TopGroups: no doc groups (SetDocGroups)");
        if (!ranges.empty() && ranges.size() != queries.size()) throw std::runtime_error("TopGroups: one list of ranges per query, or none");
        std::vector<uint32_t> rng_ptr{0}, req_ptr{0}, exc_ptr{0}, req_terms, exc_terms;
        std::vector<ss_doc_range> rng;
        for (auto& rs : ranges) {
            for (auto& r : rs) rng.push_back(ss_doc_range{r.field, 0, r.lo, r.hi});
            rng_ptr.push_back((uint32_t)rng.size());
        }
        if (!rng.empty() && !has_doc_fields) throw std::runtime_error("TopGroups: no doc fields (SetDocFields)");
        std::vector<std::string> rewritten;
        const std::vector<std::string>* qs = &queries;
        if (query_operators) {
            auto id_of = [&](const std::string& w) -> uint32_t {
                auto it = terms.id.find(md5::hex(w));
                return it == terms.id.end() ? SS_UNKNOWN_TERM : it->second;
            };
            for (auto& q : queries) {
                const QueryOperators op = parseQueryOperators(q, laundry);
                rewritten.push_back(op.query);
                for (auto& w : op.required) req_terms.push_back(id_of(w));
                for (auto& w : op.excluded) exc_terms.push_back(id_of(w));
                req_ptr.push_back((uint32_t)req_terms.size());
                exc_ptr.push_back((uint32_t)exc_terms.size());
            }
            qs = &rewritten;
        }
        const Tokenised t = tokenise(*qs, nullptr, false);
        if (!t.p_terms.empty()) throw std::runtime_error("TopGroups: quoted phrases are not counted");
        const size_t nq = (size_t)t.nq, mm = (size_t)std::max(m, 1);
        std::vector<ss_group_count> rows(nq * mm);
        std::vector<int32_t> n_page(nq);
        std::vector<uint32_t> n_groups(nq), n_ungrouped(nq), n_match(nq);
        check(ss_top_groups(scorer, t.nq, t.q_ptr.data(), t.q_terms.data(), nullptr, query_operators ? req_ptr.data() : nullptr, req_terms.data(),
                            query_operators ? exc_ptr.data() : nullptr, exc_terms.data(), ranges.empty() ? nullptr : rng_ptr.data(), rng.data(),
                            first, m, rows.data(), n_page.data(), n_groups.data(), n_ungrouped.data(), n_match.data()), "ss_top_groups");
        std::vector<GroupPage> out(nq);
        for (size_t q = 0; q < nq; q++) {
            out[q].Total = n_match[q];
            out[q].Groups = n_groups[q];
            out[q].Ungrouped = n_ungrouped[q];
            for (int32_t r = 0; r < n_page[q]; r++) {
                const ss_group_count& g = rows[q * mm + (size_t)r];
                out[q].Rows.emplace_back(doc_group_names.at(g.group), g.count);
            }
        }
        return out;
    }
private:
    // What FieldStats and FieldHistogram pass for M(q): the tokenised queries, the clauses of ranges[q] and, with SetQueryOperators, the
    // "+word" / "-word" terms, read as in FacetCounts.  A query string with a quoted phrase is refused.
    struct MatchQuery {
        Tokenised t;
        std::vector<uint32_t> rng_ptr{0}, req_ptr{0}, exc_ptr{0}, req_terms, exc_terms;
        std::vector<ss_doc_range> rng;
    };
    MatchQuery match_query(const char* who, const std::vector<std::string>& queries, const std::vector<std::vector<FieldRange>>& ranges) {
        using namespace spaghetti;
        if (!has_doc_fields) throw std::runtime_error(std::string(who) + ": no doc fields (SetDocFields)");
        if (!ranges.empty() && ranges.size() != queries.size()) throw std::runtime_error(std::string(who) + ": one list of ranges per query, or none");
        MatchQuery mq;
        for (auto& rs : ranges) {
            for (auto& r : rs) mq.rng.push_back(ss_doc_range{r.field, 0, r.lo, r.hi});
            mq.rng_ptr.push_back((uint32_t)mq.rng.size());
        }
        std::vector<std::string> rewritten;
        const std::vector<std::string>* qs = &queries;
        if (query_operators) {
            auto id_of = [&](const std::string& w) -> uint32_t {
                auto it = terms.id.find(md5::hex(w));
                return it == terms.id.end() ? SS_UNKNOWN_TERM : it->second;
            };
            for (auto& q : queries) {
                const QueryOperators op = parseQueryOperators(q, laundry);
                rewritten.push_back(op.query);
                for (auto& w : op.required) mq.req_terms.push_back(id_of(w));
                for (auto& w : op.excluded) mq.exc_terms.push_back(id_of(w));
                mq.req_ptr.push_back((uint32_t)mq.req_terms.size());
                mq.exc_ptr.push_back((uint32_t)mq.exc_terms.size());
            }
            qs = &rewritten;
        }
        mq.t = tokenise(*qs, nullptr, false);
        if (!mq.t.p_terms.empty()) throw std::runtime_error(std::string(who) + ": quoted phrases are not counted");
        return mq;
    }
public:
    // The range, the exact sum and the missing count of doc fields over ALL docs every query matches (ss_field_stats): the docs FacetCounts
    // counts under the clauses of ranges[q] (an empty `ranges`: none for any query); fields: at most SS_MAX_DOC_FIELDS field numbers.
    std::vector<FieldStatsRow> FieldStats(const std::vector<std::string>& queries, const std::vector<std::vector<FieldRange>>& ranges,
                                          const std::vector<int32_t>& fields) {
        using namespace spaghetti;
        const MatchQuery mq = match_query("FieldStats", queries, ranges);
        const size_t nq = (size_t)mq.t.nq, nf = fields.size();
        std::vector<ss_field_stat> stats(nq * std::max<size_t>(nf, 1));
        std::vector<uint32_t> n_match(nq);
        check(ss_field_stats(scorer, mq.t.nq, mq.t.q_ptr.data(), mq.t.q_terms.data(), nullptr, query_operators ? mq.req_ptr.data() : nullptr,
                             mq.req_terms.data(), query_operators ? mq.exc_ptr.data() : nullptr, mq.exc_terms.data(),
                             ranges.empty() ? nullptr : mq.rng_ptr.data(), mq.rng.data(), (int32_t)nf, nf ? fields.data() : nullptr, stats.data(),
                             n_match.data()), "ss_field_stats");
        std::vector<FieldStatsRow> out(nq);
        for (size_t q = 0; q < nq; q++) {
            out[q].Total = n_match[q];
            for (size_t i = 0; i < nf; i++) {
                const ss_field_stat& s = stats[q * nf + i];
                FieldStat f;
                f.Min = s.min; f.Max = s.max; f.SumLo = s.sum_lo; f.SumHi = s.sum_hi; f.Count = s.count; f.Missing = s.missing;
                out[q].Fields.push_back(f);
            }
        }
        return out;
    }
    // The matches per bin of a doc field over ALL docs every query matches (ss_field_histogram), "matches per month": bin b holds
    // origin + b * width <= value < origin + (b + 1) * width; with edges, edges[b] <= value < edges[b + 1] (n_bins = edges.size() - 1,
    // strictly ascending).  n_bins <= SS_MAX_HIST_BINS.
    std::vector<FieldHistogramRow> FieldHistogram(const std::vector<std::string>& queries, const std::vector<std::vector<FieldRange>>& ranges,
                                                  int field, int64_t origin, uint64_t width, int n_bins) {
        return field_histogram(queries, ranges, field, origin, width, nullptr, n_bins);
    }
    std::vector<FieldHistogramRow> FieldHistogram(const std::vector<std::string>& queries, const std::vector<std::vector<FieldRange>>& ranges,
                                                  int field, const std::vector<int64_t>& edges) {
        if (edges.size() < 2) throw std::runtime_error("FieldHistogram: at least two edges");
        return field_histogram(queries, ranges, field, 0, 1, edges.data(), (int)(edges.size() - 1));
    }
private:
    std::vector<FieldHistogramRow> field_histogram(const std::vector<std::string>& queries, const std::vector<std::vector<FieldRange>>& ranges,
                                                   int field, int64_t origin, uint64_t width, const int64_t* edges, int n_bins) {
        using namespace spaghetti;
        const MatchQuery mq = match_query("FieldHistogram", queries, ranges);
        const size_t nq = (size_t)mq.t.nq, nb = (size_t)std::max(n_bins, 1);
        std::vector<uint32_t> counts(nq * nb);
        std::vector<ss_hist_tail> tails(nq);
        check(ss_field_histogram(scorer, mq.t.nq, mq.t.q_ptr.data(), mq.t.q_terms.data(), nullptr, query_operators ? mq.req_ptr.data() : nullptr,
                                 mq.req_terms.data(), query_operators ? mq.exc_ptr.data() : nullptr, mq.exc_terms.data(),
                                 ranges.empty() ? nullptr : mq.rng_ptr.data(), mq.rng.data(), field, origin, width, edges, n_bins, counts.data(),
                                 tails.data()), "ss_field_histogram");
        std::vector<FieldHistogramRow> out(nq);
        for (size_t q = 0; q < nq; q++) {
            out[q].Total = tails[q].n_match;
            out[q].Below = tails[q].below;
            out[q].Above = tails[q].above;
            out[q].Missing = tails[q].missing;
            out[q].Counts.assign(counts.begin() + q * nb, counts.begin() + (q + 1) * nb);
        }
        return out;
    }
public:
    // RetrieveBatch sorted by a doc field (SetDocFields): page [first, first + k) of the first k_window rows of every query's ranking,
    // sorted stably by the field, ascending or descending ("newest first": field 0, descending).  Query operators are not read here.
    std::vector<FieldSortedPage> SortByField(const std::vector<std::string>& queries, int field, bool descending, int k_window, int first = 0,
                                             int k = 50, const std::vector<std::map<std::string, double>>* topicProbs = nullptr,
                                             bool live_topic_probs = false) {
        using namespace spaghetti;
        if (!has_doc_fields) throw std::runtime_error("SortByField: no doc fields (SetDocFields)");
        if (query_operators) throw std::runtime_error("SortByField: query operators are not read here (SetQueryOperators(false))");
        if (prefix_expansions) throw std::runtime_error("SortByField: prefix queries are not read here (SetPrefixQueries(0))");
        const Tokenised t = tokenise(queries, topicProbs, live_topic_probs);
        const size_t nq = (size_t)t.nq, kk = (size_t)std::max(k, 1);
        std::vector<ss_hit> rows(nq * (size_t)std::max(k_window, 1)), page(nq * kk);
        std::vector<int32_t> n_rows(nq), n_page(nq);
        std::vector<int64_t> values(nq * kk);
        check(ss_score_topk_phrase(scorer, t.nq, t.q_ptr.data(), t.q_terms.data(), t.p_ptr.data(), t.p_terms.data(), t.q_len.data(),
                                   t.probs.empty() ? nullptr : t.probs.data(), k_window, rows.data(), n_rows.data()), "ss_score_topk_phrase");
        check(ss_sort_hits_by_field(scorer, t.nq, k_window, rows.data(), n_rows.data(), field, descending ? 1 : 0, first, k, page.data(),
                                    n_page.data(), values.data()), "ss_sort_hits_by_field");
        const std::vector<std::vector<Rank_combined>> ranks = to_ranks(t.nq, k, page, n_page);
        std::vector<FieldSortedPage> out(nq);
        for (size_t q = 0; q < nq; q++) {
            out[q].Results = ranks[q];
            out[q].Values.assign(values.begin() + q * kk, values.begin() + q * kk + n_page[q]);
        }
        return out;
    }
    // RetrieveBatch without near-duplicate pages (SetNearDuplicates): page [first, first + k) of every query's ranking after the
    // rows whose body signature agrees with an earlier kept row's in at least min_match slots have been dropped, taken over the
    // first k_window rows of the ranking (k_window <= SS_MAX_TOPK; 1 <= min_match <= the signatures' slots).  The rows are scored
    // by ss_score_topk_phrase and go through ss_dedup_hits.  Query operators are not read here.
    std::vector<DedupedPage> RetrieveBatchDeduped(const std::vector<std::string>& queries, int k_window, int min_match, int first = 0,
                                                  int k = 50, const std::vector<std::map<std::string, double>>* topicProbs = nullptr,
                                                  bool live_topic_probs = false) {
        using namespace spaghetti;
        if (!signatures_built) throw std::runtime_error("RetrieveBatchDeduped: no signatures (SetNearDuplicates)");
        if (query_operators) throw std::runtime_error("RetrieveBatchDeduped: query operators are not read here (SetQueryOperators(false))");
        if (prefix_expansions) throw std::runtime_error("RetrieveBatchDeduped: prefix queries are not read here (SetPrefixQueries(0))");
        const Tokenised t = tokenise(queries, topicProbs, live_topic_probs);
        const size_t nq = (size_t)t.nq, kk = (size_t)std::max(k, 1);
        std::vector<ss_hit> page(nq * kk), rows(nq * (size_t)std::max(k_window, 1));
        std::vector<int32_t> n_page(nq), n_kept(nq), n_rows(nq);
        std::vector<uint32_t> similar(nq * kk);
        check(ss_score_topk_phrase(scorer, t.nq, t.q_ptr.data(), t.q_terms.data(), t.p_ptr.data(), t.p_terms.data(), t.q_len.data(),
                                   t.probs.empty() ? nullptr : t.probs.data(), k_window, rows.data(), n_rows.data()), "ss_score_topk_phrase");
        check(ss_dedup_hits(scorer, t.nq, k_window, rows.data(), n_rows.data(), min_match, first, k, page.data(), n_page.data(), similar.data(),
                            n_kept.data()), "ss_dedup_hits");
        const std::vector<std::vector<Rank_combined>> ranks = to_ranks(t.nq, k, page, n_page);
        std::vector<DedupedPage> out(nq);
        for (size_t q = 0; q < nq; q++) {
            out[q].Results = ranks[q];
            out[q].Similar.assign(similar.begin() + q * kk, similar.begin() + q * kk + n_page[q]);
            out[q].Kept = n_kept[q];
        }
        return out;
    }
    // The same in two halves, for a caller that has the next batch ready while this one runs (RetrieveBatcher): BeginBatch tokenises
    // and enqueues (ss_score_topk_submit; up to SS_SCORE_INFLIGHT batches), FinishBatch waits for that batch and converts its rows.
    struct PendingBatch { uint64_t ticket = 0; int nq = 0, k = 0; };
    PendingBatch BeginBatch(const std::vector<std::string>& queries, int k = 50) {
        using namespace spaghetti;
        const Tokenised t = tokenise(queries, nullptr, false);
        PendingBatch pb;
        pb.nq = t.nq;
        pb.k = k;
        check(ss_score_topk_submit(scorer, t.nq, t.q_ptr.data(), t.q_terms.data(), t.p_ptr.data(), t.p_terms.data(), t.q_len.data(), nullptr, k,
                                   &pb.ticket), "ss_score_topk_submit");
        return pb;
    }
    std::vector<std::vector<Rank_combined>> FinishBatch(const PendingBatch& pb) {
        using namespace spaghetti;
        std::vector<ss_hit> hits((size_t)pb.nq * pb.k + 1);
        std::vector<int32_t> n_hits((size_t)pb.nq + 1);
        check(ss_score_topk_collect(scorer, pb.ticket, hits.data(), n_hits.data()), "ss_score_topk_collect");
        return to_ranks(pb.nq, pb.k, hits, n_hits);
    }
};

// Request batching in front of the device.  The reference serves every HTTP request in its own
// goroutine (cmd/server/server.go:47) and each runs its own Retrieve; here concurrent callers are collected for at most
// `max_wait` (or until `max_batch` are waiting) and answered by ONE ss_score_topk_phrase call.  Retrieve() blocks its
// caller like the reference's function does and returns that caller's own result.
class RetrieveBatcher {
public:
    RetrieveBatcher(DeviceIndex& di, int k = 50, std::chrono::microseconds max_wait = std::chrono::microseconds(1000), size_t max_batch = 1024)
        : di_(di), k_(k), max_wait_(max_wait), max_batch_(max_batch), worker_([this] { run(); }) {}
    ~RetrieveBatcher() {
        { std::lock_guard<std::mutex> lk(mu_); stop_ = true; }
        cv_.notify_all();
        worker_.join();
    }
    std::vector<Rank_combined> Retrieve(const std::string& query) {
        std::future<std::vector<Rank_combined>> fut;
        {
            std::lock_guard<std::mutex> lk(mu_);
            pending_.emplace_back(query, std::promise<std::vector<Rank_combined>>());
            fut = pending_.back().second.get_future();
        }
        cv_.notify_all();
        return fut.get();               // rethrows what the batch call threw (the reference panics)
    }
    size_t batches() const { return n_batches_; }
    size_t largest_batch() const { return largest_; }

private:
    typedef std::vector<std::pair<std::string, std::promise<std::vector<Rank_combined>>>> Batch;
    struct InFlight { DeviceIndex::PendingBatch pb; Batch batch; };
    // every caller of `batch` that has no answer yet is served on its own: only the caller of an offending query gets the error
    // (done[i]: caller i has its answer — a promise takes exactly one value or exception: a second set_* throws future_error,
    // which inside a catch block would end the serving thread)
    void one_by_one(Batch& batch, std::vector<char>& done) {
        for (size_t i = 0; i < batch.size(); i++) {
            if (done[i]) continue;
            std::exception_ptr err;
            try {
                auto one = di_.RetrieveBatch({batch[i].first}, k_);
                if (one.size() != 1) throw std::runtime_error("RetrieveBatch: no result for a single query");
                batch[i].second.set_value(std::move(one[0]));
                done[i] = 1;
            } catch (...) {
                err = std::current_exception();
            }
            if (!done[i]) {
                try { batch[i].second.set_exception(err); } catch (...) {}   // promise already satisfied: nothing left to tell
                done[i] = 1;
            }
        }
    }
    void finish(InFlight& f) {
        std::vector<char> done(f.batch.size(), 0);
        bool whole = true;
        try {
            auto res = di_.FinishBatch(f.pb);
            if (res.size() != f.batch.size()) throw std::runtime_error("RetrieveBatch: result count differs from the batch");
            for (size_t i = 0; i < f.batch.size(); i++) {
                f.batch[i].second.set_value(std::move(res[i]));
                done[i] = 1;
            }
        } catch (...) {
            whole = false;
        }
        if (!whole) one_by_one(f.batch, done);
    }
    // Up to TWO batches in flight: while the device scores batch i, this thread tokenises and enqueues batch i+1 (if callers are
    // waiting), then hands batch i back.  With nobody waiting a batch is handed back as soon as it is done, as before.
    void run() {
        std::deque<InFlight> flight;
        for (;;) {
            Batch batch;
            {
                std::unique_lock<std::mutex> lk(mu_);
                if (flight.empty()) {
                    cv_.wait(lk, [this] { return stop_ || !pending_.empty(); });
                    if (stop_ && pending_.empty()) return;
                    // first request in: wait a little for company
                    const auto deadline = std::chrono::steady_clock::now() + max_wait_;
                    cv_.wait_until(lk, deadline, [this] { return stop_ || pending_.size() >= max_batch_; });
                }
                batch.swap(pending_);                                      // (a batch is running: whoever waits now rides the next one)
            }
            if (!batch.empty()) {
                std::vector<std::string> queries;
                for (auto& p : batch) queries.push_back(p.first);
                n_batches_++;
                largest_ = std::max(largest_, batch.size());
                InFlight f;
                bool begun = true;
                try {
                    f.pb = di_.BeginBatch(queries, k_);
                } catch (...) {
                    begun = false;                                         // the library refuses the batch as a whole (e.g. one phrase beyond SS_MAX_PHRASE_TERMS)
                }
                if (begun) {
                    f.batch = std::move(batch);
                    flight.push_back(std::move(f));
                } else {
                    std::vector<char> done(batch.size(), 0);
                    one_by_one(batch, done);
                }
            }
            // hand back the oldest batch when a second one is behind it, or when nobody is waiting to be batched
            bool more;
            { std::lock_guard<std::mutex> lk(mu_); more = !pending_.empty(); }
            while (!flight.empty() && (flight.size() >= 2 || !more)) {
                finish(flight.front());
                flight.pop_front();
            }
        }
    }
    DeviceIndex& di_;
    int k_;
    std::chrono::microseconds max_wait_;
    size_t max_batch_;
    std::mutex mu_;
    std::condition_variable cv_;
    std::vector<std::pair<std::string, std::promise<std::vector<Rank_combined>>>> pending_;
    bool stop_ = false;
    size_t n_batches_ = 0, largest_ = 0;
    std::thread worker_;
};

// retrieval.Retrieve(query, ctx, forw, inv) []Rank_combined — main_retrieve.go:15; first 50 (:99-103)
inline std::vector<Rank_combined> Retrieve(const std::string& query, db::Context& ctx, std::vector<db::DB*>& forw, std::vector<db::DB*>& inv) {
    static DeviceIndex* dev = nullptr;      // loaded on first use, like the server's long-lived tables
    static std::vector<db::DB*>* loaded_for = nullptr;
    if (!dev || loaded_for != &inv) {
        delete dev;
        dev = new DeviceIndex();
        dev->load(ctx, forw, inv);
        loaded_for = &inv;
    }
    return dev->RetrieveBatch({query}, 50)[0];
}

}  // namespace retrieval
