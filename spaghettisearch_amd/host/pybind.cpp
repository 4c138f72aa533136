// pybind.cpp — Python binding of the C++ host layer (module spaghettisearch_amd._host), so that the
// pytest parity tests can drive the reference-shaped entry points:
//   ranking.UpdateTopicSensitivePagerank / ranking.UpdateTermWeights / retrieval.Retrieve
// over in-memory tables holding the reference's JSON row formats.
#include <pybind11/functional.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include "retrieval.hpp"

namespace py = pybind11;

PYBIND11_MODULE(_host, m) {
    m.doc() = "C++ host mirror of SpaghettiSearch's ranking/retrieval entry points above the HIP C ABI";
    py::class_<db::MemDB>(m, "MemDB")
        .def(py::init<>())
        .def("set", [](db::MemDB& d, const std::string& k, const std::string& v) { d.rows[k] = v; })
        .def("get", [](db::MemDB& d, const std::string& k) {
            auto it = d.rows.find(k);
            if (it == d.rows.end()) throw py::key_error(k);
            return it->second;
        })
        .def("keys", [](db::MemDB& d) {
            std::vector<std::string> out;
            for (auto& kv : d.rows) out.push_back(kv.first);
            return out;
        })
        .def("__len__", [](db::MemDB& d) { return d.rows.size(); })
        .def("clear", [](db::MemDB& d) { d.rows.clear(); });

    py::class_<retrieval::Rank_combined>(m, "Rank_combined")
        .def_readonly("DocHash", &retrieval::Rank_combined::DocHash)
        .def_readonly("PageRank", &retrieval::Rank_combined::PageRank)
        .def_readonly("FinalRank", &retrieval::Rank_combined::FinalRank)
        .def_readonly("TitleRank", &retrieval::Rank_combined::TitleRank)
        .def_readonly("BodyRank", &retrieval::Rank_combined::BodyRank);

    py::class_<retrieval::ResultProximity>(m, "ResultProximity")
        .def_readonly("HasSpan", &retrieval::ResultProximity::HasSpan)
        .def_readonly("Start", &retrieval::ResultProximity::Start)
        .def_readonly("End", &retrieval::ResultProximity::End)
        .def_readonly("Words", &retrieval::ResultProximity::Words)
        .def_readonly("Present", &retrieval::ResultProximity::Present)
        .def_readonly("Occurrences", &retrieval::ResultProximity::Occurrences);
    py::class_<retrieval::RankedPage>(m, "RankedPage")
        .def_readonly("Results", &retrieval::RankedPage::Results)
        .def_readonly("Scores", &retrieval::RankedPage::Scores);
    py::class_<retrieval::ProximityPage>(m, "ProximityPage")
        .def_readonly("Results", &retrieval::ProximityPage::Results)
        .def_readonly("Scores", &retrieval::ProximityPage::Scores)
        .def_readonly("Spans", &retrieval::ProximityPage::Spans);
    py::class_<retrieval::ResultPassage>(m, "ResultPassage")
        .def_readonly("HasPassage", &retrieval::ResultPassage::HasPassage)
        .def_readonly("Start", &retrieval::ResultPassage::Start)
        .def_readonly("Last", &retrieval::ResultPassage::Last)
        .def_readonly("Words", &retrieval::ResultPassage::Words)
        .def_readonly("Distinct", &retrieval::ResultPassage::Distinct)
        .def_readonly("Occurrences", &retrieval::ResultPassage::Occurrences);
    py::class_<retrieval::WordSuggestion>(m, "WordSuggestion")
        .def_readonly("Token", &retrieval::WordSuggestion::Token)
        .def_readonly("Words", &retrieval::WordSuggestion::Words)
        .def_readonly("Distances", &retrieval::WordSuggestion::Distances)
        .def_readonly("Freqs", &retrieval::WordSuggestion::Freqs);
    py::class_<retrieval::WordCompletion>(m, "WordCompletion")
        .def_readonly("Word", &retrieval::WordCompletion::Word)
        .def_readonly("Freq", &retrieval::WordCompletion::Freq);
    py::class_<retrieval::ResultExplanation>(m, "ResultExplanation")
        .def_readonly("TitleWords", &retrieval::ResultExplanation::TitleWords)
        .def_readonly("BodyWords", &retrieval::ResultExplanation::BodyWords)
        .def_readonly("MissingWords", &retrieval::ResultExplanation::MissingWords)
        .def_property_readonly("FirstPosition", [](const retrieval::ResultExplanation& e) -> py::object {
            return e.HasPosition ? py::object(py::float_(e.FirstPosition)) : py::object(py::none());
        });

    py::class_<retrieval::CollapsedPage>(m, "CollapsedPage")
        .def_readonly("Results", &retrieval::CollapsedPage::Results)
        .def_readonly("Same", &retrieval::CollapsedPage::Same)
        .def_readonly("Kept", &retrieval::CollapsedPage::Kept);
    py::class_<retrieval::FieldSortedPage>(m, "FieldSortedPage")
        .def_readonly("Results", &retrieval::FieldSortedPage::Results)
        .def_readonly("Values", &retrieval::FieldSortedPage::Values);
    py::class_<retrieval::FacetCount>(m, "FacetCount")
        .def_readonly("Total", &retrieval::FacetCount::Total)
        .def_readonly("Masks", &retrieval::FacetCount::Masks)
        .def_readonly("Buckets", &retrieval::FacetCount::Buckets);
    py::class_<retrieval::GroupPage>(m, "GroupPage")
        .def_readonly("Total", &retrieval::GroupPage::Total)
        .def_readonly("Groups", &retrieval::GroupPage::Groups)
        .def_readonly("Ungrouped", &retrieval::GroupPage::Ungrouped)
        .def_readonly("Rows", &retrieval::GroupPage::Rows);
    py::class_<retrieval::FieldStat>(m, "FieldStat")
        .def_readonly("Min", &retrieval::FieldStat::Min)
        .def_readonly("Max", &retrieval::FieldStat::Max)
        .def_readonly("SumLo", &retrieval::FieldStat::SumLo)
        .def_readonly("SumHi", &retrieval::FieldStat::SumHi)
        .def_readonly("Count", &retrieval::FieldStat::Count)
        .def_readonly("Missing", &retrieval::FieldStat::Missing)
        .def("Mean", &retrieval::FieldStat::Mean);
    py::class_<retrieval::FieldStatsRow>(m, "FieldStatsRow")
        .def_readonly("Total", &retrieval::FieldStatsRow::Total)
        .def_readonly("Fields", &retrieval::FieldStatsRow::Fields);
    py::class_<retrieval::FieldHistogramRow>(m, "FieldHistogramRow")
        .def_readonly("Total", &retrieval::FieldHistogramRow::Total)
        .def_readonly("Below", &retrieval::FieldHistogramRow::Below)
        .def_readonly("Above", &retrieval::FieldHistogramRow::Above)
        .def_readonly("Missing", &retrieval::FieldHistogramRow::Missing)
        .def_readonly("Counts", &retrieval::FieldHistogramRow::Counts);
    py::class_<retrieval::VectorHit>(m, "VectorHit")
        .def_readonly("DocHash", &retrieval::VectorHit::DocHash)
        .def_readonly("Score", &retrieval::VectorHit::Score);
    py::class_<retrieval::VectorRerankedPage>(m, "VectorRerankedPage")
        .def_readonly("Results", &retrieval::VectorRerankedPage::Results)
        .def_readonly("Scores", &retrieval::VectorRerankedPage::Scores);
    py::class_<retrieval::DiversifiedPage>(m, "DiversifiedPage")
        .def_readonly("Results", &retrieval::DiversifiedPage::Results)
        .def_readonly("Rel", &retrieval::DiversifiedPage::Rel)
        .def_readonly("Sim", &retrieval::DiversifiedPage::Sim);
    py::class_<retrieval::HybridParams>(m, "HybridParams")
        .def(py::init<>())
        .def_readwrite("weighted", &retrieval::HybridParams::weighted)
        .def_readwrite("rrf_c", &retrieval::HybridParams::rrf_c)
        .def_readwrite("w_lex", &retrieval::HybridParams::w_lex)
        .def_readwrite("w_vec", &retrieval::HybridParams::w_vec);
    py::class_<retrieval::HybridPage>(m, "HybridPage")
        .def_readonly("Results", &retrieval::HybridPage::Results)
        .def_readonly("Scores", &retrieval::HybridPage::Scores)
        .def_readonly("VecScores", &retrieval::HybridPage::VecScores)
        .def_readonly("LexRanks", &retrieval::HybridPage::LexRanks)
        .def_readonly("VecRanks", &retrieval::HybridPage::VecRanks)
        .def_readonly("Union", &retrieval::HybridPage::Union);
    py::class_<retrieval::DedupedPage>(m, "DedupedPage")
        .def_readonly("Results", &retrieval::DedupedPage::Results)
        .def_readonly("Similar", &retrieval::DedupedPage::Similar)
        .def_readonly("Kept", &retrieval::DedupedPage::Kept);

    auto as_dbs = [](std::vector<db::MemDB*>& v) {
        std::vector<db::DB*> out;
        for (auto* p : v) out.push_back(p);
        return out;
    };
    m.def("UpdateTopicSensitivePagerank", [as_dbs](double d, double eps, std::vector<db::MemDB*> forward, bool teleport_sets,
                                                   std::vector<db::MemDB*> inv, bool two_vectors) {
        db::Context ctx;
        auto f = as_dbs(forward), i = as_dbs(inv);
        ranking::TopicSensitive ts;
        ts.teleport_sets = teleport_sets;
        ts.inv = &i;
        ts.two_vectors = two_vectors;
        ranking::UpdateTopicSensitivePagerank(ctx, d, eps, f, ts);
    }, py::arg("dampingFactor"), py::arg("convergenceCriterion"), py::arg("forward"), py::arg("teleport_sets") = false,
       py::arg("inv") = std::vector<db::MemDB*>(), py::arg("two_vectors") = false);
    m.def("TopicTeleportSets", [as_dbs](std::vector<db::MemDB*> forward, std::vector<db::MemDB*> inv) {
        db::Context ctx;
        auto f = as_dbs(forward), i = as_dbs(inv);
        return ranking::TopicTeleportSets(ctx, f, i);
    });
    py::class_<ranking::ResidentPagerank>(m, "ResidentPagerank")
        .def(py::init<>())
        .def("Build", [as_dbs](ranking::ResidentPagerank& r, std::vector<db::MemDB*> forward) {
            db::Context ctx;
            auto f = as_dbs(forward);
            r.Build(ctx, f);
        })
        .def("ApplyDelta", [as_dbs](ranking::ResidentPagerank& r, std::vector<db::MemDB*> forward, const std::vector<std::string>& parents) {
            db::Context ctx;
            auto f = as_dbs(forward);
            r.ApplyDelta(ctx, f, parents);
        })
        .def("Run", [as_dbs](ranking::ResidentPagerank& r, double d, double eps, std::vector<db::MemDB*> forward) {
            db::Context ctx;
            auto f = as_dbs(forward);
            r.Run(ctx, d, eps, f);
        })
        .def("SetLinkKey", &ranking::ResidentPagerank::SetLinkKey, py::arg("topic") = std::string())
        .def("TopLinks", [](ranking::ResidentPagerank& r, const std::vector<std::string>& docHashes, int32_t dir, int32_t m) {
            auto l = r.TopLinks(docHashes, dir, m);
            return py::make_tuple(l.links, l.degree);
        }, py::arg("docHashes"), py::arg("dir"), py::arg("m") = 5)
        .def_readonly("name", &ranking::ResidentPagerank::name)
        .def_readonly("rebuilds", &ranking::ResidentPagerank::rebuilds);
    auto page_info = [](const py::dict& d) {
        retrieval::PageIndexInfo p;
        p.docHash = d["docHash"].cast<std::string>();
        if (d.contains("title")) p.title = d["title"].cast<std::map<std::string, std::vector<float>>>();
        if (d.contains("body")) p.body = d["body"].cast<std::map<std::string, std::vector<float>>>();
        if (d.contains("anchors")) p.anchors = d["anchors"].cast<std::map<std::string, std::map<std::string, std::vector<float>>>>();
        if (d.contains("children")) p.children = d["children"].cast<std::vector<std::string>>();
        return p;
    };
    m.def("UpdateTermWeights", [as_dbs](db::MemDB* inv, std::vector<db::MemDB*> forw, const std::string& info) {
        db::Context ctx;
        auto f = as_dbs(forw);
        db::DB* i = inv;
        ranking::UpdateTermWeights(ctx, &i, f, info);
    }, py::arg("inv"), py::arg("forw"), py::arg("info"));
    m.def("md5_hex", &md5::hex);
    m.def("parseQueryOperators", [](const std::string& query) {
        const retrieval::QueryOperators op = retrieval::parseQueryOperators(query);
        return py::make_tuple(op.query, op.required, op.excluded);
    }, py::arg("query"));
    m.def("computeTopicProbs", [as_dbs](std::vector<db::MemDB*> inv, std::vector<db::MemDB*> forw, const std::vector<std::string>& tokens, bool as_written) {
        db::Context ctx;
        auto i = as_dbs(inv), f = as_dbs(forw);
        try {
            return retrieval::computeTopicProbs(ctx, i, f, tokens, as_written);
        } catch (const db::KeyNotFound&) {
            throw py::key_error("query word not in inv[2] (the reference panics, main_retrieve.go:120-121)");
        }
    }, py::arg("inv"), py::arg("forw"), py::arg("queryTokenised"), py::arg("as_written") = true);

    py::class_<retrieval::DeviceIndex>(m, "DeviceIndex")
        .def(py::init<>())
        .def("load", [as_dbs](retrieval::DeviceIndex& di, std::vector<db::MemDB*> forw, std::vector<db::MemDB*> inv) {
            db::Context ctx;
            auto f = as_dbs(forw), i = as_dbs(inv);
            di.load(ctx, f, i);
        })
        .def("RetrieveBatch", [](retrieval::DeviceIndex& di, const std::vector<std::string>& queries, int k,
                                 py::object topic_probs, bool live_topic_probs) {
            if (topic_probs.is_none()) return di.RetrieveBatch(queries, k, nullptr, live_topic_probs);
            auto tp = topic_probs.cast<std::vector<std::map<std::string, double>>>();
            return di.RetrieveBatch(queries, k, &tp, live_topic_probs);
        }, py::arg("queries"), py::arg("k") = 50, py::arg("topic_probs") = py::none(), py::arg("live_topic_probs") = false)
        .def("RetrieveBatch", [](retrieval::DeviceIndex& di, const std::vector<std::string>& queries, const std::vector<std::string>& masks,
                                 int k, py::object topic_probs, bool live_topic_probs) {
            if (topic_probs.is_none()) return di.RetrieveBatch(queries, masks, k, nullptr, live_topic_probs);
            auto tp = topic_probs.cast<std::vector<std::map<std::string, double>>>();
            return di.RetrieveBatch(queries, masks, k, &tp, live_topic_probs);
        }, py::arg("queries"), py::arg("masks"), py::arg("k") = 50, py::arg("topic_probs") = py::none(), py::arg("live_topic_probs") = false)
        .def("SetDocMasks", &retrieval::DeviceIndex::SetDocMasks, py::arg("sets"))
        .def("SetDocGroups", &retrieval::DeviceIndex::SetDocGroups, py::arg("keys"))
        .def("RetrieveBatchCollapsed", [](retrieval::DeviceIndex& di, const std::vector<std::string>& queries, int k_window, int g, int first,
                                          int k, py::object topic_probs, bool live_topic_probs) {
            if (topic_probs.is_none()) return di.RetrieveBatchCollapsed(queries, k_window, g, first, k, nullptr, live_topic_probs);
            auto tp = topic_probs.cast<std::vector<std::map<std::string, double>>>();
            return di.RetrieveBatchCollapsed(queries, k_window, g, first, k, &tp, live_topic_probs);
        }, py::arg("queries"), py::arg("k_window"), py::arg("g"), py::arg("first") = 0, py::arg("k") = 50,
           py::arg("topic_probs") = py::none(), py::arg("live_topic_probs") = false)
        .def("SetDocFields", &retrieval::DeviceIndex::SetDocFields, py::arg("fields"))
        .def("RetrieveBatchFiltered", [](retrieval::DeviceIndex& di, const std::vector<std::string>& queries,
                                         const std::vector<std::vector<std::tuple<int32_t, int64_t, int64_t>>>& ranges, int k,
                                         py::object topic_probs, bool live_topic_probs) {
            std::vector<std::vector<retrieval::FieldRange>> rs(ranges.size());
            for (size_t q = 0; q < ranges.size(); q++)
                for (auto& r : ranges[q]) rs[q].push_back(retrieval::FieldRange{std::get<0>(r), std::get<1>(r), std::get<2>(r)});
            if (topic_probs.is_none()) return di.RetrieveBatchFiltered(queries, rs, k, nullptr, live_topic_probs);
            auto tp = topic_probs.cast<std::vector<std::map<std::string, double>>>();
            return di.RetrieveBatchFiltered(queries, rs, k, &tp, live_topic_probs);
        }, py::arg("queries"), py::arg("ranges"), py::arg("k") = 50, py::arg("topic_probs") = py::none(), py::arg("live_topic_probs") = false)
        .def("FacetCounts", [](retrieval::DeviceIndex& di, const std::vector<std::string>& queries,
                               const std::vector<std::vector<std::tuple<int32_t, int64_t, int64_t>>>& ranges,
                               const std::vector<std::tuple<int32_t, int64_t, int64_t>>& buckets) {
            std::vector<std::vector<retrieval::FieldRange>> rs(ranges.size());
            for (size_t q = 0; q < ranges.size(); q++)
                for (auto& r : ranges[q]) rs[q].push_back(retrieval::FieldRange{std::get<0>(r), std::get<1>(r), std::get<2>(r)});
            std::vector<retrieval::FieldRange> bs;
            for (auto& b : buckets) bs.push_back(retrieval::FieldRange{std::get<0>(b), std::get<1>(b), std::get<2>(b)});
            return di.FacetCounts(queries, rs, bs);
        }, py::arg("queries"), py::arg("ranges") = std::vector<std::vector<std::tuple<int32_t, int64_t, int64_t>>>{},
           py::arg("buckets") = std::vector<std::tuple<int32_t, int64_t, int64_t>>{})
        .def("RetrieveBatchByField", [](retrieval::DeviceIndex& di, const std::vector<std::string>& queries,
                                        const std::vector<std::vector<std::tuple<int32_t, int64_t, int64_t>>>& ranges, int field, bool descending,
                                        int first, int k) {
            std::vector<std::vector<retrieval::FieldRange>> rs(ranges.size());
            for (size_t q = 0; q < ranges.size(); q++)
                for (auto& r : ranges[q]) rs[q].push_back(retrieval::FieldRange{std::get<0>(r), std::get<1>(r), std::get<2>(r)});
            return di.RetrieveBatchByField(queries, rs, field, descending, first, k);
        }, py::arg("queries"), py::arg("ranges"), py::arg("field"), py::arg("descending") = false, py::arg("first") = 0, py::arg("k") = 50)
        .def("TopGroups", [](retrieval::DeviceIndex& di, const std::vector<std::string>& queries,
                             const std::vector<std::vector<std::tuple<int32_t, int64_t, int64_t>>>& ranges, int first, int m) {
            std::vector<std::vector<retrieval::FieldRange>> rs(ranges.size());
            for (size_t q = 0; q < ranges.size(); q++)
                for (auto& r : ranges[q]) rs[q].push_back(retrieval::FieldRange{std::get<0>(r), std::get<1>(r), std::get<2>(r)});
            return di.TopGroups(queries, rs, first, m);
        }, py::arg("queries"), py::arg("ranges") = std::vector<std::vector<std::tuple<int32_t, int64_t, int64_t>>>{}, py::arg("first") = 0,
           py::arg("m") = 10)
        .def("FieldStats", [](retrieval::DeviceIndex& di, const std::vector<std::string>& queries,
                              const std::vector<std::vector<std::tuple<int32_t, int64_t, int64_t>>>& ranges, const std::vector<int32_t>& fields) {
            std::vector<std::vector<retrieval::FieldRange>> rs(ranges.size());
            for (size_t q = 0; q < ranges.size(); q++)
                for (auto& r : ranges[q]) rs[q].push_back(retrieval::FieldRange{std::get<0>(r), std::get<1>(r), std::get<2>(r)});
            return di.FieldStats(queries, rs, fields);
        }, py::arg("queries"), py::arg("ranges"), py::arg("fields"))
        .def("FieldHistogram", [](retrieval::DeviceIndex& di, const std::vector<std::string>& queries,
                                  const std::vector<std::vector<std::tuple<int32_t, int64_t, int64_t>>>& ranges, int field, int64_t origin,
                                  uint64_t width, int n_bins, py::object edges) {
            std::vector<std::vector<retrieval::FieldRange>> rs(ranges.size());
            for (size_t q = 0; q < ranges.size(); q++)
                for (auto& r : ranges[q]) rs[q].push_back(retrieval::FieldRange{std::get<0>(r), std::get<1>(r), std::get<2>(r)});
            if (edges.is_none()) return di.FieldHistogram(queries, rs, field, origin, width, n_bins);
            return di.FieldHistogram(queries, rs, field, edges.cast<std::vector<int64_t>>());
        }, py::arg("queries"), py::arg("ranges"), py::arg("field"), py::arg("origin") = 0, py::arg("width") = 1, py::arg("n_bins") = 1,
           py::arg("edges") = py::none())
        .def("SortByField", [](retrieval::DeviceIndex& di, const std::vector<std::string>& queries, int field, bool descending, int k_window,
                               int first, int k, py::object topic_probs, bool live_topic_probs) {
            if (topic_probs.is_none()) return di.SortByField(queries, field, descending, k_window, first, k, nullptr, live_topic_probs);
            auto tp = topic_probs.cast<std::vector<std::map<std::string, double>>>();
            return di.SortByField(queries, field, descending, k_window, first, k, &tp, live_topic_probs);
        }, py::arg("queries"), py::arg("field"), py::arg("descending"), py::arg("k_window"), py::arg("first") = 0, py::arg("k") = 50,
           py::arg("topic_probs") = py::none(), py::arg("live_topic_probs") = false)
        .def("SetDocVectors", &retrieval::DeviceIndex::SetDocVectors, py::arg("vectors"))
        .def("VectorSearch", &retrieval::DeviceIndex::VectorSearch, py::arg("queryVectors"), py::arg("k") = 50,
             py::arg("masks") = std::vector<std::string>())
        .def("SetVectorLists", &retrieval::DeviceIndex::SetVectorLists, py::arg("n_lists"), py::arg("centroids"))
        .def("VectorSearchProbed", &retrieval::DeviceIndex::VectorSearchProbed, py::arg("queryVectors"), py::arg("k") = 50,
             py::arg("n_probe") = 8, py::arg("masks") = std::vector<std::string>())
        .def("RerankByVector", &retrieval::DeviceIndex::RerankByVector, py::arg("queryVectors"), py::arg("rows"), py::arg("first") = 0,
             py::arg("k") = 50)
        .def("SetDocTokens", &retrieval::DeviceIndex::SetDocTokens, py::arg("tokens"))
        .def("RerankByMaxSim", &retrieval::DeviceIndex::RerankByMaxSim, py::arg("queryTokens"), py::arg("rows"), py::arg("first") = 0,
             py::arg("k") = 50)
        .def("MaxSimSearch", &retrieval::DeviceIndex::MaxSimSearch, py::arg("queryTokens"), py::arg("k") = 50,
             py::arg("masks") = std::vector<std::string>())
        .def("DiversifyByVector", &retrieval::DeviceIndex::DiversifyByVector, py::arg("queryVectors"), py::arg("rows"), py::arg("w_rel"),
             py::arg("w_div"), py::arg("first") = 0, py::arg("k") = 50)
        .def("ScoreDocs", [](retrieval::DeviceIndex& di, const std::string& query, const std::vector<std::string>& docHashes) {
            return di.ScoreDocs(query, docHashes);
        }, py::arg("query"), py::arg("docHashes"))
        .def("HybridSearch", [](retrieval::DeviceIndex& di, const std::vector<std::string>& queries, const std::vector<std::vector<int8_t>>& queryVectors,
                                int k_window, const retrieval::HybridParams& params, int first, int k, const std::vector<std::string>& masks) {
            return di.HybridSearch(queries, queryVectors, k_window, params, first, k, masks);
        }, py::arg("queries"), py::arg("queryVectors"), py::arg("k_window"), py::arg("params") = retrieval::HybridParams(), py::arg("first") = 0,
           py::arg("k") = 50, py::arg("masks") = std::vector<std::string>())
        .def("SetNearDuplicates", &retrieval::DeviceIndex::SetNearDuplicates, py::arg("n_slots"))
        .def("NearDuplicateSlots", &retrieval::DeviceIndex::NearDuplicateSlots)
        .def("RetrieveBatchDeduped", [](retrieval::DeviceIndex& di, const std::vector<std::string>& queries, int k_window, int min_match,
                                        int first, int k, py::object topic_probs, bool live_topic_probs) {
            if (topic_probs.is_none()) return di.RetrieveBatchDeduped(queries, k_window, min_match, first, k, nullptr, live_topic_probs);
            auto tp = topic_probs.cast<std::vector<std::map<std::string, double>>>();
            return di.RetrieveBatchDeduped(queries, k_window, min_match, first, k, &tp, live_topic_probs);
        }, py::arg("queries"), py::arg("k_window"), py::arg("min_match"), py::arg("first") = 0, py::arg("k") = 50,
           py::arg("topic_probs") = py::none(), py::arg("live_topic_probs") = false)
        .def("SetQueryOperators", &retrieval::DeviceIndex::SetQueryOperators, py::arg("on"))
        .def("SetSimilarPages", &retrieval::DeviceIndex::SetSimilarPages, py::arg("on"))
        .def("DocTopTerms", &retrieval::DeviceIndex::DocTopTerms, py::arg("docHash"), py::arg("m") = 5)
        .def("SimilarPages", [](retrieval::DeviceIndex& di, const std::string& docHash, int k, int m) { return di.SimilarPages(docHash, k, m); },
             py::arg("docHash"), py::arg("k") = 50, py::arg("m") = 5)
        .def("SimilarPages", [](retrieval::DeviceIndex& di, const std::string& docHash, const std::string& mask, int k, int m) {
            return di.SimilarPages(docHash, mask, k, m);
        }, py::arg("docHash"), py::arg("mask"), py::arg("k") = 50, py::arg("m") = 5)
        .def("RelatedTerms", &retrieval::DeviceIndex::RelatedTerms, py::arg("query"), py::arg("m") = 10, py::arg("k_fb") = 10, py::arg("m_doc") = 5)
        .def("ExplainResults", &retrieval::DeviceIndex::ExplainResults, py::arg("query"), py::arg("results"))
        .def("BestPassages", &retrieval::DeviceIndex::BestPassages, py::arg("query"), py::arg("results"), py::arg("width") = 20)
        .def("HitProximity", &retrieval::DeviceIndex::HitProximity, py::arg("query"), py::arg("results"))
        .def("RetrieveBatchProximity", [](retrieval::DeviceIndex& di, const std::vector<std::string>& queries, int k_window, double w_rank,
                                          double w_prox, int first, int k) {
            return di.RetrieveBatchProximity(queries, k_window, w_rank, w_prox, first, k);
        }, py::arg("queries"), py::arg("k_window"), py::arg("w_rank") = 1.0, py::arg("w_prox") = 1.0, py::arg("first") = 0, py::arg("k") = 50)
        .def("SetRankModel", &retrieval::DeviceIndex::SetRankModel, py::arg("linear"), py::arg("base"), py::arg("tree_ptr"), py::arg("nodes"))
        .def("RetrieveBatchRanked", [](retrieval::DeviceIndex& di, const std::vector<std::string>& queries, int k_window, int first, int k) {
            return di.RetrieveBatchRanked(queries, k_window, first, k);
        }, py::arg("queries"), py::arg("k_window"), py::arg("first") = 0, py::arg("k") = 50)
        .def("HasDocView", &retrieval::DeviceIndex::HasDocView)
        .def("SetLexicon", [](retrieval::DeviceIndex& di, db::MemDB* forw0) {
            db::Context ctx;
            di.SetLexicon(ctx, forw0);
        }, py::arg("forw0"))
        .def("HasLexicon", &retrieval::DeviceIndex::HasLexicon)
        .def("WordList", [](retrieval::DeviceIndex& di, const std::string& pre, int64_t first, int k) {
            py::list out;
            for (auto& w : di.WordList(pre, first, k)) out.append(py::bytes(w));       // words are bytes: not every prefix cut is UTF-8
            return out;
        }, py::arg("pre"), py::arg("first") = 0, py::arg("k") = 50)
        .def("SuggestWords", &retrieval::DeviceIndex::SuggestWords, py::arg("query"), py::arg("max_dist") = 2, py::arg("m") = 5)
        .def("Complete", &retrieval::DeviceIndex::Complete, py::arg("pre"), py::arg("m") = 10, py::arg("min_freq") = 1)
        .def("SetPrefixQueries", &retrieval::DeviceIndex::SetPrefixQueries, py::arg("expansions"))
        .def("LoadTopics", [as_dbs](retrieval::DeviceIndex& di, std::vector<db::MemDB*> forw, std::vector<db::MemDB*> inv) {
            db::Context ctx;
            auto f = as_dbs(forw), i = as_dbs(inv);
            di.LoadTopics(ctx, f, i);
        })
        .def("liveTopicProbs", &retrieval::DeviceIndex::liveTopicProbs)
        .def("ApplyDelta", [as_dbs, page_info](retrieval::DeviceIndex& di, std::vector<db::MemDB*> forw, std::vector<db::MemDB*> inv,
                                               const py::dict& before, const py::dict& after, bool update_magnitudes) {
            db::Context ctx;
            auto f = as_dbs(forw), i = as_dbs(inv);
            di.ApplyDelta(ctx, f, i, page_info(before), page_info(after), update_magnitudes);
        }, py::arg("forw"), py::arg("inv"), py::arg("before"), py::arg("after"), py::arg("update_magnitudes") = true)
        .def("ReloadPrior", [as_dbs](retrieval::DeviceIndex& di, std::vector<db::MemDB*> forw) {
            db::Context ctx;
            auto f = as_dbs(forw);
            di.ReloadPrior(ctx, f);
        })
        .def("save_snapshot", &retrieval::DeviceIndex::save_snapshot)
        .def("load_snapshot", &retrieval::DeviceIndex::load_snapshot)
        .def_readonly("categories", &retrieval::DeviceIndex::categories);
    py::class_<retrieval::RetrieveBatcher>(m, "RetrieveBatcher")
        .def(py::init([](retrieval::DeviceIndex& di, int k, int max_wait_us, size_t max_batch) {
                 return new retrieval::RetrieveBatcher(di, k, std::chrono::microseconds(max_wait_us), max_batch);
             }), py::arg("index"), py::arg("k") = 50, py::arg("max_wait_us") = 1000, py::arg("max_batch") = 1024, py::keep_alive<1, 2>())
        .def("Retrieve", [](retrieval::RetrieveBatcher& b, const std::string& q) {
            py::gil_scoped_release rel;          // other Python threads queue their requests meanwhile
            return b.Retrieve(q);
        })
        .def_property_readonly("batches", &retrieval::RetrieveBatcher::batches)
        .def_property_readonly("largest_batch", &retrieval::RetrieveBatcher::largest_batch);
    m.def("Retrieve", [as_dbs](const std::string& query, std::vector<db::MemDB*> forw, std::vector<db::MemDB*> inv) {
        db::Context ctx;
        auto f = as_dbs(forw), i = as_dbs(inv);
        retrieval::DeviceIndex di;          // the binding keeps no global state: load per call
        di.load(ctx, f, i);
        return di.RetrieveBatch({query}, 50)[0];
    });
}
