#include "Blackjack.h"

#include <cstddef>

namespace {
constexpr int WORD_MAX = (1 << 24) - 1;
constexpr int HAND_MAX = 31 + 32 + 64 * 10;   // 703
constexpr uint32_t CARD_TAG = 0x21u;

int clampi(float v, int hi) { return v >= 0.0f ? (v >= static_cast<float>(hi) ? hi : static_cast<int>(v)) : 0; }   // a NaN becomes 0

struct Hand { int t, ace, show; };
// the hand word clamped into 0..703, then its fields: t into 2..31, show into 1..10
Hand handOf(const float* st) {
    const int h = clampi(st[0], HAND_MAX);
    const int t = h & 31, show = h >> 6;
    return { t < 2 ? 2 : t, (h >> 5) & 1, show < 1 ? 1 : show };
}
int usable(const Hand& h) { return (h.ace && h.t + 10 <= 21) ? 1 : 0; }
int soft(int total, bool ace) { return total + ((ace && total + 10 <= 21) ? 10 : 0); }
}  // namespace

std::array<uint32_t, 4> Blackjack::philox4x32_10(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) {
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = static_cast<uint64_t>(0xD2511F53u) * c0, p1 = static_cast<uint64_t>(0xCD9E8D57u) * c2;
        const uint32_t n0 = static_cast<uint32_t>(p1 >> 32) ^ c1 ^ k0, n1 = static_cast<uint32_t>(p1);
        const uint32_t n2 = static_cast<uint32_t>(p0 >> 32) ^ c3 ^ k1, n3 = static_cast<uint32_t>(p0);
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return { c0, c1, c2, c3 };
}

int Blackjack::card(uint32_t word) {
    const int c = 1 + static_cast<int>((static_cast<uint64_t>(word) * 13u) >> 32);
    return c < 10 ? c : 10;
}

// one Philox call per card here: the twin states the rule, the device keeps a call's four words while consecutive indices share index >> 2
int Blackjack::cardAt(uint32_t k0, uint32_t k1, uint32_t index) {
    return card(philox4x32_10(k0, k1, index >> 2, 0u, 0u, CARD_TAG)[static_cast<size_t>(index & 3u)]);
}

float Blackjack::transition(float* st, int action, bool& terminated, int* drawn) {
    Hand h = handOf(st);
    const int n = clampi(st[1], WORD_MAX), k0 = clampi(st[2], WORD_MAX), k1 = clampi(st[3], WORD_MAX);
    const uint32_t u0 = static_cast<uint32_t>(k0), u1 = static_cast<uint32_t>(k1);
    const int a = action < 0 ? 0 : (action > 1 ? 1 : action);
    uint32_t next = static_cast<uint32_t>(n);
    float reward = -1.0f;
    int drew = 0;
    terminated = true;
    if (h.t <= 21) {   // a bust hand is reachable through an injected state only: nothing is drawn, the state stays
        if (a == 1) {
            const int c = cardAt(u0, u1, next++);
            h.t += c;
            h.ace |= c == 1 ? 1 : 0;
            terminated = h.t > 21;
            reward = h.t > 21 ? -1.0f : 0.0f;
        } else {
            const int hidden = cardAt(u0, u1, 3u);
            int dt = h.show + hidden;
            bool dace = h.show == 1 || hidden == 1;
            for (int d = 0; d < DEALER_DRAWS; d++) {   // a bound, not a `while` on data: ten cards take any two-card start to 17
                if (soft(dt, dace) < 17) {
                    const int c = cardAt(u0, u1, next++);
                    dt += c;
                    dace = dace || c == 1;
                    drew++;
                }
            }
            const int dealer = dt > 21 ? 0 : soft(dt, dace);
            const int player = h.t + 10 * usable(h);
            reward = player > dealer ? 1.0f : (player == dealer ? 0.0f : -1.0f);
        }
    }
    if (drawn) *drawn = drew;
    st[0] = static_cast<float>(h.t + 32 * h.ace + 64 * h.show);
    st[1] = static_cast<float>(next < static_cast<uint32_t>(WORD_MAX) ? static_cast<int>(next) : WORD_MAX);
    st[2] = static_cast<float>(k0);
    st[3] = static_cast<float>(k1);
    return reward;
}

void Blackjack::observe(const float* st, float* obs) {
    const Hand h = handOf(st);
    const int u = usable(h);
    for (int k = 0; k < OBS; k++) obs[k] = 0.0f;
    obs[h.t + 10 * u] = 1.0f;
    obs[32 + h.show] = 1.0f;
    obs[43 + u] = 1.0f;
}

Blackjack::Blackjack(int64_t seed, int64_t env_index) : state(4, 0.0f), episode_length(0), episode_reward(0.0f), m_seed(seed), m_env_index(env_index) {
    state[0] = 2.0f + 64.0f;   // a legal hand in front of the first reset
}

std::vector<float> Blackjack::observation() const {
    std::vector<float> obs(static_cast<size_t>(OBS));
    observe(state.data(), obs.data());
    return obs;
}

std::tuple<std::vector<float>, float, bool, bool> Blackjack::step(int64_t action) {
    bool terminated = false;
    const int a = action < 0 ? 0 : (action > 1 ? 1 : static_cast<int>(action));
    const float reward = transition(state.data(), a, terminated);
    episode_length += 1;
    episode_reward += reward;
    return { observation(), reward, terminated, false };
}

// The device's reset map: reset number k of env e under `seed` draws philox4x32_10(seed; e, k, 0, 1) and keeps the top 24 bits of its first two words as the
// key; the key's call 0 deals the player's two cards, the dealer's showing card and the hidden one
std::vector<float> Blackjack::reset() {
    const uint64_t s = static_cast<uint64_t>(m_seed);
    const std::array<uint32_t, 4> w = philox4x32_10(static_cast<uint32_t>(s), static_cast<uint32_t>(s >> 32), static_cast<uint32_t>(m_env_index),
                                                    static_cast<uint32_t>(m_resets++), 0u, 1u);
    const uint32_t k0 = w[0] >> 8, k1 = w[1] >> 8;
    const std::array<uint32_t, 4> c = philox4x32_10(k0, k1, 0u, 0u, 0u, CARD_TAG);
    const int c0 = card(c[0]), c1 = card(c[1]), show = card(c[2]);
    state = { static_cast<float>(c0 + c1 + ((c0 == 1 || c1 == 1) ? 32 : 0) + 64 * show), 4.0f, static_cast<float>(k0), static_cast<float>(k1) };
    episode_length = 0;
    episode_reward = 0.0f;
    return observation();
}
