// std::make_heap under the reference's comparison (a.value > b.value || isnan(a.value)) over values read from stdin: prints the heap
// (value bits, index) in array order.  tests/test_half16_cpu.py compares the C restatement of that algorithm with it.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

struct Item { float value; uint32_t idx; };

int main()
{
    std::vector<Item> h;
    unsigned bits;
    while (std::scanf("%x", &bits) == 1) {
        Item it;
        uint32_t b = bits;
        std::memcpy(&it.value, &b, 4);
        it.idx = (uint32_t)h.size();
        h.push_back(it);
    }
    std::make_heap(h.begin(), h.end(), [](const Item &a, const Item &b) { return (a.value > b.value) || std::isnan(a.value); });
    for (const Item &it : h) {
        uint32_t b;
        std::memcpy(&b, &it.value, 4);
        std::printf("%08x %u\n", b, it.idx);
    }
    return 0;
}
