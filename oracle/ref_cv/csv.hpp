// Stand-in for the csv-parser header line2Dup.h includes (test infrastructure).  Only Timer::displayCSV names it, and
// the match half never calls that; the writer joins a row with commas.
#ifndef SBM_REF_CSV_HPP
#define SBM_REF_CSV_HPP
#include <sstream>
#include <string>
#include <vector>

namespace csv {
namespace internals {
template <typename T> std::string to_string(T v) {
    std::ostringstream s;
    s << v;
    return s.str();
}
}  // namespace internals

template <typename OS> class Writer {
public:
    explicit Writer(OS& os) : os_(os) {}
    template <typename T> Writer& operator<<(const std::vector<T>& row) {
        for (size_t i = 0; i < row.size(); ++i) os_ << (i ? "," : "") << row[i];
        os_ << "\n";
        return *this;
    }

private:
    OS& os_;
};
template <typename OS> Writer<OS> make_csv_writer(OS& os) { return Writer<OS>(os); }
}  // namespace csv
#endif
